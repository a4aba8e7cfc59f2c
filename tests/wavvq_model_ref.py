"""vq-wav2vec's feature extractor and Gumbel quantiser head restated with torch modules - nn.Conv1d, nn.GroupNorm(1, C),
nn.Linear - from the description in qpgesture_amd/wavvq.py's docstring (fairseq is not used and not needed).  Runs in f32 or
f64 on any device; the f64 CPU run is what tests/golden/make_golden_wavvq_model.py stores, the f32 run is the yardstick
the device kernels' error is measured in."""
import numpy as np
import torch
from torch import nn

from qpgesture_amd.wavlm import conv_layers_of
from qpgesture_amd.wavvq import _as_dict


class WavVQRef(nn.Module):
    def __init__(self, args, sd, dtype=torch.float64, device="cpu"):
        super().__init__()
        a = _as_dict(args)
        self.G, self.V = a["vq_groups"], a["vq_vars"]
        layers, cin = [], 1
        for C, k, s in conv_layers_of(a):
            layers.append(nn.Sequential(nn.Conv1d(cin, C, k, stride=s, bias=False), nn.Dropout(0.0),
                                        nn.GroupNorm(1, C, eps=1e-5, affine=not a["non_affine_group_norm"]), nn.ReLU()))
            cin = C
        self.conv_layers = nn.ModuleList(layers)
        if a["vq_depth"] == 2:
            H = np.asarray(sd["vector_quantizer.weight_proj.0.0.weight"]).shape[0]
            self.weight_proj = nn.Sequential(nn.Sequential(nn.Linear(cin, H), nn.ReLU()), nn.Linear(H, self.G * self.V))
        else:
            self.weight_proj = nn.Linear(cin, self.G * self.V)
        own = self.state_dict()
        for name in own:
            src = ("feature_extractor." + name) if name.startswith("conv_layers.") else ("vector_quantizer." + name)
            own[name] = torch.as_tensor(np.asarray(sd[src]))
        self.load_state_dict(own)
        self.to(dtype=dtype, device=device).eval()
        self.dtype = dtype

    @torch.no_grad()
    def features(self, wav):
        """(B, n) -> z (B, T, C), channels last like the device code (fairseq keeps (B, C, T))."""
        x = torch.as_tensor(wav).to(dtype=self.dtype, device=next(self.parameters()).device).unsqueeze(1)
        for layer in self.conv_layers:
            x = layer(x)
        x = (x.abs() + 1).log()
        return x.transpose(1, 2).contiguous()

    @torch.no_grad()
    def logits(self, wav):
        z = self.features(wav)
        return self.weight_proj(z).view(z.shape[0], z.shape[1], self.G, self.V)

    @torch.no_grad()
    def forward_idx(self, wav):
        return self.logits(wav).max(dim=-1)[1]


# The recorded cases (tests/golden/wavvq_model.npz): name -> (geometry, weight seed, wav seed, B, n, gain, silent window).
# n = 465 is the vq-wav2vec stack's receptive field, ONE frame (464 samples give none); 945 - the figure the feature's
# issue names for that edge - gives 4 frames and is kept as a case of its own; 3 200 and 4 001 give 639 and 799 layer-0
# frames, both odd; "silent" puts an all-zero window in a batch next to a loud one; "full" is the real geometry.
SEED_TINY, SEED_FULL = 40, 43
CASES = {
    "n465": ("tiny", SEED_TINY, 51, 2, 465, 1.0, None),
    "n945": ("tiny", SEED_TINY, 52, 2, 945, 1.0, None),
    "n3200": ("tiny", SEED_TINY, 53, 2, 3200, 1.0, None),
    "n4001": ("tiny", SEED_TINY, 54, 3, 4001, 1.0, None),
    "silent": ("tiny", SEED_TINY, 55, 2, 3200, 3.0, 0),
    "full": ("gumbel", SEED_FULL, 56, 1, 64000, 1.0, None),
}
FULL_ROWS = np.arange(0, 398, 50)       # the frames of the full-size case whose z and logits rows are stored
_sd_cache = {}


def geometry(kind):
    from qpgesture_amd import synth
    return synth.WAVVQ_TINY if kind == "tiny" else synth.WAVVQ_GUMBEL


def case_inputs(name):
    """(geometry, state dict, wav (B, n) f32) of a recorded case, regenerated from its seeds."""
    from qpgesture_amd import synth
    kind, seed_w, seed_wav, B, n, gain, silent = CASES[name]
    if (kind, seed_w) not in _sd_cache:
        _sd_cache[(kind, seed_w)] = synth.make_wavvq_state_dict(seed_w, geometry(kind))
    wav = synth.make_wav(seed_wav, B, n) * np.float32(gain)
    if silent is not None:
        wav[silent] = 0.0
    return geometry(kind), _sd_cache[(kind, seed_w)], wav


def top2_margin(logits):
    """Gap between the largest and the second largest value of each (frame, group): (B, T, G)."""
    top = torch.as_tensor(logits).topk(2, dim=-1)[0]
    return (top[..., 0] - top[..., 1]).cpu().numpy()
