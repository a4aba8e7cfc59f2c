"""Where does the conv kernel's time go?  Times the B=256 encode (variant "0") or the f64 audio sweep (variant "a0") of
the product library, or the encode of a library given by path.  (The variants with parts of the K loop compiled out
needed the -DQPG_CONV_PROBE / -DQPG_AUDIO_PROBE hooks: see README.md.)"""
import os, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
variant = sys.argv[1]
import qpgesture_amd._lib as L
if variant.endswith(".so"):
    L.LIB_PATH = os.path.abspath(variant)
import torch
if variant == "a0":
    N, Q, T, F, G = 2048, 48, 180, 1024, 26
    dev = torch.device("cuda:0")
    base = torch.randn((N, T, F), device=dev)
    q32 = torch.randn((Q, 6 * F), device=dev)
    qn2 = (q32.double() ** 2).sum(1)
    cn2 = torch.rand((N, G), device=dev, dtype=torch.float64) + 6000
    cand_t = torch.arange(G, device=dev, dtype=torch.int32) * 6
    D = torch.empty((Q, N * G), device=dev, dtype=torch.float64)
    run = lambda: L.call("qpg_audio_cosine_f64", dev, base, N, T, F, cand_t, G, 6, 2, cn2, q32, qn2, Q, D, D.stride(0))
    for _ in range(3): run()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(10): run()
    torch.cuda.synchronize(); ms = (time.perf_counter() - t0) / 10 * 1e3
    print("audio variant %s: %.1f us (%.1f TF-equivalent)" % (variant, ms * 1e3, 2.0 * Q * N * G * 6 * F / ms / 1e9))
    sys.exit(0)
from qpgesture_amd import synth
from qpgesture_amd.vqvae import VQVAE
dev = torch.device("cuda:0")
m = VQVAE(None, 135, device=dev).load_state_dict(synth.make_vqvae_state_dict(7))
x = torch.randn((256, 240, 135), device=dev)
for _ in range(2): m.encode(x)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(10): m.encode(x)
torch.cuda.synchronize(); te = (time.perf_counter() - t0) / 10
print("variant %s: encode B=256 %.3f ms (%.1f TF-equivalent)" % (variant, te * 1e3, 1.639e9 * 256 / te / 1e12))
