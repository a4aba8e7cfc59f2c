"""CPU tests of the host logic and of the C-ABI library surface (no compute calls without a GPU)."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

from qpgesture_amd import _lib, synth
from qpgesture_amd import code_knn as ck
from qpgesture_amd import data_processing as dp


def test_library_loads_and_exports_every_declared_symbol():
    lib = _lib.load()
    names = _lib.declared_symbols()
    assert len(names) >= 16 and "qpg_audio_cosine_f64" in names and "qpg_match_steps" in names
    for n in names:
        assert hasattr(lib, n), "include/qpg.h declares %s but libqpg_hip.so does not export it" % n
    assert lib.qpg_version() >= 107
    import os
    assert lib.qpg_dev_kernarg() == (1 if os.environ.get("HIP_FORCE_DEV_KERNARG") == "1" else 0)


def test_bindings_cover_the_header():
    """load() leaves no declared function at ctypes' defaults: each carries the argtypes and restype the header parser
    derived, and every launch - (qpg_ctx*, void* stream, ...) - returns int."""
    lib, protos = _lib.load(), _lib.prototypes()
    assert set(_lib.declared_symbols()) | set(_lib.debug_hook_symbols()) == set(protos)
    assert not set(_lib.declared_symbols()) & set(_lib.debug_hook_symbols())
    launches = 0
    for name in _lib.declared_symbols():
        fn, proto = getattr(lib, name), protos[name]
        assert fn.argtypes is not None and list(fn.argtypes) == proto.argtypes, name
        assert fn.restype is proto.restype, name
        if proto.on_stream:
            assert fn.restype is ctypes.c_int and list(fn.argtypes[:2]) == [ctypes.c_void_p] * 2, name
            launches += 1
    assert launches >= 88 and protos["qpg_audio_cosine_f64"].on_stream and not protos["qpg_ctx_create"].on_stream


def test_pinned_prototypes():
    """Six prototypes written out as literals, one per shape the header -> ctypes mapping has to get right (a parser bug
    that is also a bug of the tests around it can not hide behind these)."""
    lib = _lib.load()
    P, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    want = {
        "qpg_audio_cosine_f64": (I, [P, P, P, I, I, I, P, I, I, I, P, P, P, I, P, L]),
        "qpg_percode_select_mixed_f64_cut": (I, [P, P, P, I, L, I, P, L, I, D, ctypes.c_int32, P, P, P, I, L, P, I, I, P, I, I,
                                                 I, P, P, P, D, D, P, P, L, I, P, P, I, I]),
        "qpg_hl_rows_bytes": (L, [L, I]),                       # int64_t return and parameter
        "qpg_last_error": (I, [P, ctypes.c_size_t]),            # size_t
        "qpg_ctx_create": (I, [I, P]),                          # pointer to pointer
        "qpg_build_id": (ctypes.c_char_p, []),                  # const char*, no parameters
    }
    for name, (restype, argtypes) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert ctypes.sizeof(L) == 8 and ctypes.sizeof(I) == 4 and ctypes.sizeof(ctypes.c_size_t) == 8


def test_product_library_exports_no_debug_hooks_and_is_built_from_this_tree():
    """no global mutable state except the opaque context.  The measurement hooks (qpg_debug_*) exist only in
    -DQPG_DEBUG_HOOKS variant builds; the product library must not export any of them - and it must be the library compiled
    from THIS tree's sources: qpg_build_id() == the hash of csrc/* + include/qpg.h (build.source_hash)."""
    import subprocess
    from qpgesture_amd import build
    lib = _lib.load()
    hooks = _lib.debug_hook_symbols()
    assert "qpg_debug_gemm64_waves" in hooks and "qpg_debug_convt_shape" in hooks
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "qpg_build_id" in exported and "qpg_audio_cosine_hl" in exported
    leaked = sorted(n for n in exported if n.startswith("qpg_debug"))
    assert not leaked, "the product library exports debug hooks: %s" % leaked
    for n in hooks:
        assert not hasattr(lib, n)
    assert lib.qpg_build_id().decode() == build.source_hash() == build.lib_build_id()
    # the knobs that remain are per-context (they need a device: exercised in the GPU suite); bad arguments fail cleanly here
    assert lib.qpg_ctx_set_option(None, 0, 1) == -1 and "null context" in _lib.last_error()


def test_kernel_sources_take_no_build_knobs():
    """The product kernels are one program: no -D ablation, timer or A/B switch compiles parts of them in or out.  Every
    #if / #ifdef / #ifndef / #elif of csrc/*.hip and csrc/*.h may test the macros listed here and nothing else (in
    particular no `#ifndef X / #define X default` wrapper around a constant)."""
    import re
    from qpgesture_amd import build
    allowed = {"QPG_DEBUG_HOOKS", "QPG_BUILD_ID", "QPG_CHECK_RCCL_ABI", "QPG_HAVE_RCCL_H", "__has_include", "__cplusplus"}
    paths = [p for p in build.sources() + build.headers() if os.path.dirname(p) == build.CSRC]
    assert len(paths) >= 17
    directives, bad = 0, []
    for path in paths:
        with open(path) as f:
            for no, line in enumerate(f, 1):
                m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
                if not m:
                    continue
                directives += 1
                cond = re.sub(r"//.*|/\*.*?\*/|<[^>]*>|\"[^\"]*\"", " ", m.group(2))
                names = set(re.findall(r"[A-Za-z_]\w*", cond)) - {"defined"}
                if names - allowed:
                    bad.append("%s:%d: %s" % (os.path.basename(path), no, sorted(names - allowed)))
    assert directives >= 5                      # (the hooks blocks, the build id, the RCCL header check: the scan sees them)
    assert not bad, "conditional compilation on macros outside the allow-list:\n" + "\n".join(bad)


def test_error_reporting_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.qpg_ctx_create(0, ctypes.byref(h))
    assert rc < 0 and "qpg_ctx_create" in _lib.last_error()
    assert lib.qpg_ctx_create(0, None) == -1


def test_product_refuses_cpu_device():
    A = synth.make_db(2, 0, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ck.GestureDB(synth.make_codes(2, 1), dp.interp_wavlm(A["wavlm"]), A["context"].squeeze(2),
                     A["phase_dense"], synth.make_signature(2), device="cpu")


def test_grids_match_oracle():
    from oracle import knn_oracle as O
    for n, st in ((180, 6), (398, 398 / 30), (240, 8)):
        ks, kint, cidx = O.audio_grid(n, st)
        a, b = ck.audio_grid(n, st)
        assert a == kint and b == cidx and len(a) == 26
    ks, rows = ck.text_grid()
    assert ks == list(range(0, 208, 8)) and rows == list(range(26))
    assert [ck.phase_slot(k) for k in (0, 6, 150, 200, 331)] == [O.phase_slot(k) for k in (0, 6, 150, 200, 331)]


def test_loader_matches_oracle_windowing():
    from oracle import knn_oracle as O
    with tempfile.TemporaryDirectory() as td:
        p = synth.write_npz_set(td, 3, 2, 7, 8, 9, 10, wavlm_dim=64)
        L = dp.load_db_codebook(p["train_database"], p["train_codebook"], p["test_data"], p["train_wavlm"],
                                p["test_wavlm"], p["train_wavvq"], p["test_wavvq"])
        tr = np.load(p["train_database"], allow_pickle=True)
        assert np.array_equal(L.train_wavlm, O.interp_wavlm(np.load(p["train_wavlm"])["wavlm"]))
        assert L.train_wavlm.shape == (3, 180, 64) and L.train_wavlm.flags.c_contiguous
        assert np.array_equal(L.train_phase, O.densify_phase(tr["phase"]))
        assert np.array_equal(L.train_phase, synth.make_db(3, 7, 64)["phase_dense"])
        assert L.train_context.shape == (3, 30, 384) and L.code.shape == (3, 30)
        assert L.test_wavvq.shape == (2, 398, 2)


def test_densify_phase_accepts_dense():
    x = np.random.default_rng(0).standard_normal((2, 240, 4, 8)).astype(np.float32)
    assert np.array_equal(dp.densify_phase(x), x)


def test_checkpoint_with_pickled_easydict(tmp_path):
    """train.py:114-116 pickles an easydict.EasyDict into the checkpoint; it must load without easydict."""
    import sys
    import types
    import torch
    from qpgesture_amd.checkpoint import AttrDict, load_checkpoint
    mod = types.ModuleType("easydict")
    EasyDict = type("EasyDict", (dict,), {"__module__": "easydict", "__qualname__": "EasyDict"})
    mod.EasyDict = EasyDict
    sys.modules["easydict"] = mod
    try:
        sd = {"module.bottleneck.level_blocks.0.k": torch.arange(6.).reshape(2, 3)}
        path = str(tmp_path / "ck.bin")
        torch.save({"args": EasyDict({"VQVAE": {"width": 512}, "lr": 3e-5}), "epoch": 7, "model_dict": sd}, path)
    finally:
        del sys.modules["easydict"]
    ck = load_checkpoint(path)
    assert ck["epoch"] == 7 and isinstance(ck["args"], AttrDict) and ck["args"].lr == 3e-5
    assert ck["args"].VQVAE.width == 512 and not hasattr(ck["args"], "dilation_cycle")
    assert torch.equal(ck["model_dict"]["module.bottleneck.level_blocks.0.k"], sd["module.bottleneck.level_blocks.0.k"])
    torch.save(sd, path)                                    # bare state_dict
    assert "model_dict" in load_checkpoint(path)


def test_reference_config_loads():
    import os
    from qpgesture_amd.checkpoint import load_config
    p = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpgesture_amd", "configs",
                     "codebook.yml")
    cfg = load_config(p)
    assert cfg.VQVAE.width == 512 and cfg.VQVAE.downs_t == [3] and len(cfg.data_mean) == 135


def test_vqvae_layer_order():
    """vqvae.layer_order, the one statement of the network's layer sequence (a pure function, no device): kinds in the
    order of encdec.py, dilations growth ** d per resnet (resnet.py:57-62), reversed in the decoder on request, and the
    state-dict names in the order of the reference's state_dict()."""
    from qpgesture_amd import synth
    from qpgesture_amd.vqvae import layer_order

    def kinds(plan):
        return [l[0] for l in plan]

    def dils(plan):
        d = [l[3] for l in plan if l[0] == "res"]
        return [d[i:i + depth] for i in range(0, len(d), depth)]

    depth = 3
    enc, dec = layer_order(3, 3, 3, True)
    assert kinds(enc) == ["down", "res", "res", "res"] * 3 + ["conv3"]
    assert kinds(dec) == ["conv3"] + ["res", "res", "res", "up"] * 3 + ["conv3"]
    assert dils(enc) == [[1, 3, 9]] * 3 and dils(dec) == [[9, 3, 1]] * 3
    assert all(l[3] == 1 for l in enc + dec if l[0] != "res")
    assert [l[2] for l in enc if l[0] == "res"] == [(i, j) for i in range(3) for j in range(3)]
    assert [l[2] for l in dec if l[0] != "res"] == ["dec_in", 0, 1, 2, "dec_out"]
    assert dils(layer_order(3, 3, 3, False)[1]) == [[1, 3, 9]] * 3
    names = []                              # what the records' names expand to: the reference's parameter order
    for kind, name, _, _ in enc + dec:
        names += [name + ".model.1", name + ".model.3"] if kind == "res" else [name]
    ref = [k[7:-7] for k in synth.make_vqvae_state_dict(7) if k.endswith(".weight")]
    assert names == ref and len(names) == 45
    depth = 4
    enc, dec = layer_order(2, 4, 2, True)
    assert kinds(enc) == ["down"] + ["res"] * 4 + ["down"] + ["res"] * 4 + ["conv3"]
    assert kinds(dec) == ["conv3"] + (["res"] * 4 + ["up"]) * 2 + ["conv3"]
    assert dils(enc) == [[1, 2, 4, 8]] * 2 and dils(dec) == [[8, 4, 2, 1]] * 2
    assert dils(layer_order(2, 4, 2, False)[1]) == [[1, 2, 4, 8]] * 2


def test_training_host_logic_without_gpu():
    """Host-side pieces of the training loop that need no device: the reference-shaped initial state_dict
    (names/shapes of a fresh reference model, torch default init bounds), MultiStepLR, the CLI parser and config."""
    import torch
    from qpgesture_amd import synth, train
    from qpgesture_amd.checkpoint import load_config
    from qpgesture_amd.optim import MultiStepLR
    from qpgesture_amd.vqvae import init_state_dict
    sd = init_state_dict(seed=3)
    ref = {k[7:]: tuple(np.asarray(v).shape) for k, v in synth.make_vqvae_state_dict(7).items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref and len(sd) == 91
    w = sd["encoders.0.level_blocks.0.model.0.0.weight"]              # Conv1d(135, 512, 4): bound 1/sqrt(135*4)
    assert float(w.abs().max()) <= 1.0 / np.sqrt(135 * 4) and float(w.abs().max()) > 0.9 / np.sqrt(135 * 4)
    wt = sd["decoders.0.level_blocks.0.model.1.1.weight"]             # ConvTranspose1d(512, 512, 4): size(1)*k
    assert tuple(wt.shape) == (512, 512, 4) and float(wt.abs().max()) <= 1.0 / np.sqrt(512 * 4)
    assert float(sd["bottleneck.level_blocks.0.k"].abs().sum()) == 0.0
    assert torch.equal(init_state_dict(seed=3)["decoders.0.out.bias"], sd["decoders.0.out.bias"])

    class Opt:
        lr = 3e-5
    o = Opt()
    s = MultiStepLR(o, [100, 200], 0.1)
    lrs = []
    for _ in range(201):
        s.step()
        lrs.append(o.lr)
    assert lrs[98] == 3e-5 and abs(lrs[99] - 3e-6) < 1e-18 and abs(lrs[199] - 3e-7) < 1e-18

    a = train.parse_args(["--gpu", "1", "--synthetic", "8", "--epochs", "2"])
    assert a.gpu == "1" and a.synthetic == 8 and a.epochs == 2 and a.config.endswith("codebook.yml")
    cfg = load_config(a.config)
    assert cfg.batch_size == 256 and cfg.lr == 3e-5 and list(cfg.betas) == [0.5, 0.999] and cfg.VQVAE.l_mu == 0.99


def test_oracle_forward_loss_terms():
    """oracle/vqvae_oracle.losses against hand-computed values on a tiny sequence (vqvae.py:244-267)."""
    import torch
    from oracle import vqvae_oracle as VO
    xt = torch.tensor([[[0.0], [1.0], [3.0], [6.0]]])
    xo = torch.tensor([[[0.5], [1.0], [2.0], [6.0]]])
    loss, m = VO.losses(xt, xo, torch.tensor(2.0), hps_commit=0.02, vel=1.0, acc=1.0, reg=0.5)
    assert abs(float(m["recons_loss"]) - (0.5 + 0 + 1 + 0) / 4) < 1e-7
    # velocities: target [1,2,3], out [0.5,1,4] -> |diff| = [0.5,1,1]
    assert abs(float(m["velocity_loss"]) - 2.5 / 3) < 1e-7
    # accelerations: target [1,1], out [0.5,3] -> |diff| = [0.5,2]; regularisation = mean(out_acc^2)
    assert abs(float(m["acceleration_loss"]) - 1.25) < 1e-7
    assert abs(float(m["regularization"]) - (0.25 + 9.0) / 2) < 1e-6
    want = 0.375 + 2.0 * 0.02 + 0.5 * 4.625 + 2.5 / 3 + 1.25
    assert abs(float(loss) - want) < 1e-6


def _clang(*args):
    """The compiler the tree is built with, on C input, syntax only (it has to exist: nothing here builds without it)."""
    import subprocess
    from qpgesture_amd import build
    clang = subprocess.check_output([build.HIPCC, "-print-prog-name=clang"]).decode().strip()
    return subprocess.check_output([clang, "-x", "c", "-fsyntax-only", "-I", os.path.dirname(_lib.HEADER_PATH)]
                                   + list(args)).decode()


def _compiler_view():
    """include/qpg.h as clang's AST states it: {function: (return kind, [parameter kinds], on_stream)} over the product
    declarations and the -DQPG_DEBUG_HOOKS ones, the set of names only the latter has, and {struct typedef: field names}.
    Kinds: ptr / i32 / i64 / f32 / f64 / size_t, and cstr (a returned char*) / void for return types - typedef names are
    resolved through the AST's own typedef declarations, not by their spelling."""
    import json
    funcs, names, records = {}, [], {}
    for flags in ([], ["-DQPG_DEBUG_HOOKS"]):
        top = json.loads(_clang("-Xclang", "-ast-dump=json", *flags, _lib.HEADER_PATH))["inner"]
        typedefs = {n["name"]: n["type"].get("desugaredQualType", n["type"]["qualType"])
                    for n in top if n["kind"] == "TypedefDecl"}

        def kind(t, ret=False):
            t = t.strip()
            if t.endswith("*"):
                return "cstr" if ret and t.replace("const", "").replace(" ", "") == "char*" else "ptr"
            t = t.replace("const ", "")
            while t in typedefs:
                t = typedefs[t]
            return {"int": "i32", "long": "i64", "long long": "i64", "unsigned long": "size_t", "float": "f32",
                    "double": "f64", "void": "void"}[t]
        last_record = None
        for n in top:
            if n["kind"] == "RecordDecl":
                last_record = [f["name"] for f in n.get("inner", []) if f["kind"] == "FieldDecl"]
            elif n["kind"] == "TypedefDecl" and n["name"].startswith("qpg_") and last_record:
                records[n["name"]] = last_record             # (typedef struct { ... } qpg_x;)
            elif n["kind"] == "FunctionDecl" and n["name"].startswith("qpg_"):
                params = [(p["type"]["qualType"], p.get("name")) for p in n.get("inner", []) if p["kind"] == "ParmVarDecl"]
                on_stream = len(params) > 1 and params[0][0] == "qpg_ctx *" and params[1] == ("void *", "stream")
                ret = n["type"]["qualType"].split("(")[0]
                funcs[n["name"]] = (kind(ret, ret=True), [kind(t) for t, _ in params], on_stream)
        names.append({n["name"] for n in top if n["kind"] == "FunctionDecl" and n["name"].startswith("qpg_")})
    return funcs, names[1] - names[0], records


_CTYPES_KIND = {ctypes.c_void_p: "ptr", ctypes.c_int: "i32", ctypes.c_int64: "i64", ctypes.c_float: "f32",
                ctypes.c_double: "f64", ctypes.c_size_t: "size_t", ctypes.c_char_p: "cstr", None: "void"}


def _signature_mismatches(bound, funcs):
    """bound: {name: (restype, argtypes)} as ctypes types; funcs: _compiler_view()[0].  One line per function that differs."""
    bad = ["%s: bound but not declared" % n for n in sorted(set(bound) - set(funcs))]
    bad += ["%s: declared but not bound" % n for n in sorted(set(funcs) - set(bound))]
    for name in sorted(set(bound) & set(funcs)):
        restype, argtypes = bound[name]
        got = (_CTYPES_KIND[restype], None if argtypes is None else [_CTYPES_KIND[t] for t in argtypes])
        if got != funcs[name][:2]:
            bad.append("%s: bound as %s, the compiler says %s" % (name, got, funcs[name][:2]))
    return bad


def test_ctypes_signatures_match_the_header():
    """What load() has set on the library agrees with the COMPILER's reading of include/qpg.h (clang's AST, with and without
    -DQPG_DEBUG_HOOKS), for every declared function: arity, the kind of every parameter and the kind of the return value
    (a drifted ctypes signature would corrupt the call silently).  The hook functions, which the product library does not
    export, are held against the parser's output instead."""
    lib, protos = _lib.load(), _lib.prototypes()
    funcs, hooks, _ = _compiler_view()
    assert hooks == set(_lib.debug_hook_symbols()) and set(funcs) - hooks == set(_lib.declared_symbols())
    bound = {}
    for name, proto in protos.items():
        fn = proto if proto.hook else getattr(lib, name)
        bound[name] = (fn.restype, fn.argtypes)
    assert len(bound) >= 120
    assert _signature_mismatches(bound, funcs) == []
    assert {n for n, p in protos.items() if p.on_stream} == {n for n, f in funcs.items() if f[2]}


def _scratch_header(tmp_path, *edits):
    txt = open(_lib.HEADER_PATH).read()
    for old, new in edits:
        assert txt.count(old) == 1, old
        txt = txt.replace(old, new)
    path = str(tmp_path / "qpg.h")
    with open(path, "w") as f:
        f.write(txt)
    return path


def test_signature_check_catches_planted_errors(tmp_path):
    """The comparison above is not vacuous: a header copy with one int64_t parameter turned into int and one return type
    changed, given to the parser while the compiler reads the real header, is reported - those two functions, nothing else."""
    path = _scratch_header(tmp_path, ("int64_t qpg_hl_rows_bytes(int64_t R, int D);", "int64_t qpg_hl_rows_bytes(int R, int D);"),
                           ("int64_t qpg_vq_reduce_ws_bytes(void);", "int qpg_vq_reduce_ws_bytes(void);"))
    protos, _ = _lib.parse_header(path)
    bad = _signature_mismatches({n: (p.restype, p.argtypes) for n, p in protos.items()}, _compiler_view()[0])
    print("\n".join(bad))
    assert len(bad) == 2 and bad[0].startswith("qpg_hl_rows_bytes: ") and bad[1].startswith("qpg_vq_reduce_ws_bytes: ")


def test_parser_refuses_an_unknown_type_word(tmp_path):
    """A type the mapping does not know is an error that names the function - never a silent `int`."""
    for old, new in (("int64_t qpg_hl_rows_bytes(int64_t R, int D);", "int64_t qpg_hl_rows_bytes(uint64_t R, int D);"),
                     ("int64_t qpg_hl_rows_bytes(int64_t R, int D);", "long qpg_hl_rows_bytes(int64_t R, int D);"),
                     ("int64_t qpg_hl_rows_bytes(int64_t R, int D);", "int64_t qpg_hl_rows_bytes(int64_t R, void D);")):
        with pytest.raises(TypeError, match="qpg_hl_rows_bytes"):
            _lib.parse_header(_scratch_header(tmp_path, (old, new)))


def test_struct_mirrors_have_the_compiler_s_layout(tmp_path):
    """ConvDesc / VqModel are hand-written mirrors of qpg_conv_desc / qpg_vq_model: size, field names, field order and every
    field offset are the compiler's (clang's record layouts of the header's own typedefs)."""
    import re
    src = str(tmp_path / "layout.c")
    with open(src, "w") as f:
        f.write('#include "qpg.h"\nint use[sizeof(qpg_conv_desc) + sizeof(qpg_vq_model)];\n')
    dump = _clang("-Xclang", "-fdump-record-layouts-simple", src)
    layouts = {m.group(1): (int(m.group(2)), [int(o) for o in m.group(3).split(",")]) for m in re.finditer(
        r"Type: (\w+)\n\nLayout: <ASTRecordLayout\n\s*Size:(\d+)\n.*?FieldOffsets: \[([\d, ]+)\]>", dump, re.S)}
    fields = _compiler_view()[2]
    for cname, mirror in (("qpg_conv_desc", _lib.ConvDesc), ("qpg_vq_model", _lib.VqModel)):
        bits, offsets = layouts[cname]
        assert [n for n, _ in mirror._fields_] == fields[cname], cname
        assert ctypes.sizeof(mirror) * 8 == bits, cname
        assert [getattr(mirror, n).offset * 8 for n, _ in mirror._fields_] == offsets, cname
    assert ctypes.sizeof(_lib.ConvDesc) == 48 and ctypes.sizeof(_lib.VqModel) == 4144
    assert [getattr(_lib.ConvDesc, n).offset for n, _ in _lib.ConvDesc._fields_] == [0, 8, 16, 20, 24, 28, 32, 40]


def test_header_constants_equal_the_literals_they_replaced():
    from qpgesture_amd import code_knn, sorted_rows, vqvae
    assert _lib.QPG_MODE_PREFUSED == 0x200 and _lib.QPG_MODE_SERIAL_WALK == 0x100
    assert (code_knn.MODE_AUD_TXT, code_knn.MODE_AUD, code_knn.MODE_TXT) == (0, 1, 2)
    assert _lib.QPG_CONV16_WEXP_FROM_IMAGE == 0x7fff == vqvae.VQVAE.WEXP_FROM_IMAGE
    assert _lib.QPG_VQ_MAX_DOWN == 4 and _lib.QPG_VQ_MAX_DEPTH == 4
    assert _lib.QPG_OPT_GATE_DEDUP_FROM_CHAINS == 0
    assert code_knn.AUDIO_MX_ERR == _lib.QPG_AUDIO_MX_ERR == 2.05e-6
    assert code_knn.AUDIO_HL_ERR == sorted_rows.HL_GEMM_ERR == _lib.QPG_AUDIO_HL_ERR == 1.3e-6
    # the other shapes a value takes in the header: parenthesised, negative, a shift; integers stay integers
    assert _lib.QPG_EINVAL == -1 and _lib.QPG_PAE_MAX_CHUNK == 1 << 22 and _lib.CONSTANTS["QPG_PAET_PARAM_FLOATS"] == 1034098
    assert all(type(v) in (int, float) for v in _lib.CONSTANTS.values()) and type(_lib.QPG_PAE_MAX_CHUNK) is int
    assert "QPG_H" not in _lib.CONSTANTS


# ---------------------------------------------------------------------------------------------------------------
# round 2 host logic
# ---------------------------------------------------------------------------------------------------------------
def test_tpack_layout_matches_its_definition():
    """vqvae.tpack: out[n // nb][kb][g][n % nb][j] = W[k = 16 kb + 4 g + j][n], k = tap * cin_pad + ci, zero padded
    (what csrc/qpg_convt.hip's fragment reads and LDS-DMA stages assume)."""
    import torch
    from qpgesture_amd.vqvae import tpack
    g = torch.Generator().manual_seed(0)
    taps, cin, cout, cin_pad, nb = 3, 20, 135, 32, 128
    w = torch.randn((taps, cin, cout), generator=g)
    p = tpack(w, cin_pad, nb).view(2, taps * cin_pad // 16, 4, nb, 4)
    for (n, tap, ci) in [(0, 0, 0), (134, 2, 19), (127, 1, 7), (128, 0, 16), (5, 2, 3)]:
        k = tap * cin_pad + ci
        assert p[n // nb, k // 16, (k % 16) // 4, n % nb, k % 4] == w[tap, ci, n]
    assert float(p[1, :, :, 7:, :].abs().max()) == 0.0                      # channels >= 135 are padding
    k = 0 * cin_pad + 25                                                     # input channel >= cin is padding
    assert float(p[:, k // 16, (k % 16) // 4, :, k % 4].abs().max()) == 0.0


def test_exchange_layout_offsets():
    from qpgesture_amd.code_knn import ExchangeLayout
    lay = ExchangeLayout(96, 512, 4, ["aud", "txt"], True, "cpu")
    n = 24 * 512
    # (round 4: every block ends with an 8-byte slot whose first i32 is the sender's trouble word)
    assert lay.Qb == 24 and lay.off == {"aud_d": 0, "aud_i": 8 * n, "txt_d": 12 * n, "txt_i": 16 * n, "flags": 20 * n}
    assert lay.block_bytes == 20 * n + 8 and lay.send.numel() == 4 * (20 * n + 8)
    d, i, qb, bs = lay.views("aud")
    assert d.dtype.is_floating_point and d.element_size() == 8 and d.numel() == n and (qb, bs) == (24, 20 * n + 8)
    one = ExchangeLayout(48, 512, 1, ["aud"], False, "cpu")                 # wavvq audio: f32 distances, all-gather
    assert one.views("aud")[0].element_size() == 4 and one.views("aud")[2:] == (0, 0)
    with pytest.raises(AssertionError):
        ExchangeLayout(50, 512, 4, ["aud"], True, "cpu")


def test_savgol_tables_and_bvh_writer(tmp_path):
    """bvh.savgol_tables == scipy.signal.savgol_filter(x, 15, 2) (mode='interp'), and the minimal BVH round-trips its
    channel table."""
    from scipy.signal import savgol_filter
    from qpgesture_amd import bvh
    mid, head, tail = bvh.savgol_tables(15, 2)
    x = np.random.default_rng(0).standard_normal(40)
    want = savgol_filter(x, 15, 2)
    got = np.array([head[t] @ x[:15] if t < 7 else (tail[t - 33] @ x[25:] if t >= 33 else mid @ x[t - 7:t + 8])
                    for t in range(40)])
    assert np.abs(got - want).max() < 1e-12
    e = np.random.default_rng(1).uniform(-170, 170, size=(5, 45))
    order = bvh.write_bvh(str(tmp_path / "x.bvh"), e)
    txt = open(str(tmp_path / "x.bvh")).read().splitlines()
    assert sorted(order) == list(range(15)) and order[0] == 0
    m = txt.index("MOTION")
    rows = np.array([l.split() for l in txt[m + 3:]], float)
    cols = np.concatenate([np.arange(3 * i, 3 * i + 3) for i in order])
    assert rows.shape == (5, 45) and np.abs(rows - e[:, cols]).max() < 1e-5
    assert txt[m + 1] == "Frames: 5" and txt.count("\tEnd Site") + sum("End Site" in l for l in txt) >= 3


def test_synth_variants_plant_what_they_say():
    from qpgesture_amd import synth
    tr, te, code = synth.make_db(48, 30), synth.make_db(2, 31), synth.make_codes(48, 32)
    synth.apply_variant(tr, te, code, "neartie")
    assert np.array_equal(te["wavlm"][0], tr["wavlm"][5]) and np.array_equal(tr["wavlm"][22], tr["wavlm"][5])
    d = tr["wavlm"][20] != tr["wavlm"][5]
    assert 0 < d.mean() < 0.02 and np.array_equal(code[20], code[5]) and not np.array_equal(code[21], code[5])
    assert np.abs(tr["wavlm"][20][d] / tr["wavlm"][5][d] - 1).max() < 2e-7          # one float32 ulp
    tr2, te2, code2 = synth.make_db(48, 40), synth.make_db(2, 41), synth.make_codes(48, 42)
    synth.apply_variant(tr2, te2, code2, "texttie")
    ctx = tr2["context"].reshape(-1, 384)
    assert len(np.unique(ctx, axis=0)) < 0.7 * len(ctx)                              # many identical rows
    with pytest.raises(ValueError):
        synth.apply_variant(tr, te, code, "nope")


def test_numpy_ranks_is_the_reference_expression():
    import torch
    from qpgesture_amd.code_knn import CodeKNN
    d = torch.tensor([[0.5, 0.0, 0.0, 1e3, 0.25], [3.0, 2.0, 1.0, 0.0, 1e3]], dtype=torch.float32)
    r = CodeKNN.numpy_ranks(d).numpy()
    for row, got in zip(d.numpy(), r):
        assert np.array_equal(got, np.array(list(row.astype(np.float64))).argsort().argsort())


def test_mixed_precision_constants_agree_with_the_header():
    """The band the mixed-precision select re-evaluates in must cover twice the sweep's bound as the C side states it."""
    import re
    from qpgesture_amd import code_knn
    txt = open(_lib.HEADER_PATH).read()
    m = re.search(r"#define\s+QPG_AUDIO_MX_ERR\s+([0-9.eE+-]+)", txt)
    assert m and float(m.group(1)) == code_knn.AUDIO_MX_ERR
    assert code_knn.AUDIO_MX_BAND >= 2.0 * code_knn.AUDIO_MX_ERR
    u = 2.0 ** -24
    assert code_knn.AUDIO_MX_ERR >= 32 * u / (1 - 32 * u) + 1e-13        # gamma_32 + the f64 part
    m2 = re.search(r"#define\s+QPG_AUDIO_HL_ERR\s+([0-9.eE+-]+)", txt)
    assert m2 and float(m2.group(1)) == code_knn.AUDIO_HL_ERR and code_knn.AUDIO_HL_BAND >= 2.0 * code_knn.AUDIO_HL_ERR
    # the split-f16 sweep's budget (csrc/qpg_audio_hl.hip, audio_cosine_hl2_kernel): chains of six instructions through
    # one accumulator, the four cross-term instructions first; representation; the f32-stored matrix;
    # subnormal l planes: an absolute error <= 2^-25 per element = 2^-25 sqrt(6144) / |x|_scaled of the product of norms per
    # side, with |x|_scaled >= sqrt(HL_NORM2_MIN) - the threshold the sweeps' validity guard enforces (the
    # guard used to ask for a scaled norm >= 1 while this line divided by 2^14); f64 sums
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpgesture_amd", "csrc",
                            "qpg_audio_hl.hip")).read()
    norm2_min = float(re.search(r"#define\s+HL_NORM2_MIN\s+([0-9.eE+-]+)", src).group(1))
    assert len(re.findall(r"< HL_NORM2_MIN", src)) >= 2          # both operands of the sweep kernel
    k6 = 13 + 17 * 2.0 ** -10                       # cross instructions first: round 3's chain of two + a tiny C
    assert code_knn.AUDIO_HL_ERR >= (k6 * u + (2 * 2.0 ** -23 + u) + 2 * u +
                                     2 * 2.0 ** -25 * 6144 ** 0.5 / norm2_min ** 0.5 + 1e-13)
    # the one-plane image of an f16-stored track (round 5): the database side is exact - chains of four, the query's
    # representation and subnormals only
    assert code_knn.AUDIO_HL_ERR >= k6 * u + 2.0 ** -23 + 2 * u + 2.0 ** -25 * 6144 ** 0.5 / norm2_min ** 0.5 + 1e-13
    # the text prefilter / cfg-3 GEMM keeps round 3's kernel and bound (chains of two, separate cross accumulators)
    from qpgesture_amd import sorted_rows
    assert sorted_rows.HL_GEMM_ERR >= 13 * u + 12 * 193 * u / 2048 + (2 * 2.0 ** -23 + u) + 2 * u + 1e-13


def test_numpy_ranks_follow_the_reference_s_array_dtype():
    """the reference ranks np.array(list): float32 when every code has a (np.float32) text distance, float64 as
    soon as one `1e+3` Python float is left in the list, int64 for the Levenshtein audio (GestureKNN.py:553, 574)."""
    import torch
    from qpgesture_amd.code_knn import CodeKNN
    rng = np.random.default_rng(0)
    d = rng.standard_normal((3, 512)).astype(np.float32)
    d[:, 100:200] = d[:, :1]                                     # exact ties: the order NumPy's sort leaves is dtype business
    idx = np.zeros((3, 512), np.int32)
    idx[1, 7] = -1
    d[1, 7] = 1e3
    got = CodeKNN.numpy_ranks(torch.from_numpy(d), torch.from_numpy(idx)).numpy()
    for r in range(3):
        lst = [np.float32(x) for x in d[r]]
        if r == 1:
            lst[7] = 1e+3                                        # the reference's placeholder: a Python float
        arr = np.array(lst)
        assert arr.dtype == (np.float64 if r == 1 else np.float32)
        assert np.array_equal(got[r], arr.argsort().argsort())
    lev = rng.integers(0, 12, size=(2, 512)).astype(np.float32)
    got = CodeKNN.numpy_ranks(torch.from_numpy(lev), torch.zeros((2, 512), dtype=torch.int32), integer=True).numpy()
    for r in range(2):
        arr = np.array([int(x) for x in lev[r]])
        assert arr.dtype == np.int64 and np.array_equal(got[r], arr.argsort().argsort())


def test_status_word_is_never_ignored():
    from qpgesture_amd.code_knn import CodeKNN, GuardOverflow
    CodeKNN.check_status([0, 0])
    with pytest.raises(GuardOverflow) as e:
        CodeKNN.check_status([1, 5])                              # the guard's word outranks the IndexError
    assert e.value.flags == 5
    with pytest.raises(IndexError):
        CodeKNN.check_status([1, 0])


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus N` with WORLD_SIZE unset re-executes itself under torch.distributed.run with N ranks and
    still prints ONE JSON line (VERDICT r2 next #3a).  QPG_BENCH_LAUNCH_CHECK=1 stops every rank after the rendezvous
    (gloo all-reduce), before anything needs a GPU."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, QPG_BENCH_LAUNCH_CHECK="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "3", "--steps", "2", "--warmup", "1"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    assert json.loads(lines[0]) == {"launch_check": True, "n_gpus": 3, "rank_sum": 6}


def test_audio_object_uses_m0_only_in_the_dma_asm():
    """qpg_audio.hip issues its LDS-DMA from inline asm that sets m0 (so that hipcc's wait-count model does not see the
    DMA) and names m0 as a clobber; that is safe as long as nothing the compiler generated reads or writes m0 in that
    translation unit.  Compile it to gfx950 assembly with the product's flags and check: every m0 operand belongs to an
    `s_mov_b32 m0` inside an ASMSTART / ASMEND block."""
    import os
    import subprocess
    import tempfile
    from qpgesture_amd import build as B
    src = os.path.join(B.CSRC, "qpg_audio.hip")
    if not os.path.exists(B.HIPCC):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "a.s")
        flags = [f for f in B.FLAGS if f not in ("-shared", "-Wall")]
        subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", src, "-o", out], cwd=td,
                              stderr=subprocess.DEVNULL)
        lines = open(out).read().splitlines()
    inside, uses_out, movs = False, [], 0
    for l in lines:
        if "#ASMSTART" in l:
            inside = True
        elif "#ASMEND" in l:
            inside = False
        code = l.split(";")[0]
        if " m0" in code or ",m0" in code:
            if inside and "s_mov_b32 m0" in code:
                movs += 1
            else:
                uses_out.append(l)
    # the scan must see the DMA sites: an instantiation of audio_cosine_mx2_kernel issues the query tile at 4 places (the
    # prologue and the 3 unrolled stages), 3 one-KB pieces each = 12 moves; the launches instantiate it twice (f32 / f16 base)
    assert movs >= 2 * 12 and not uses_out, uses_out[:5]


def test_sorted_rows_drop_later_duplicates_of_a_code():
    """sorted_rows.SortedRows keeps only the FIRST of identical rows of a code (identical rows tie exactly for every query;
    first-wins picks the lowest index): the mask logic, on the CPU, with a forced hash collision path (same code, same
    hash is only possible for equal rows here, so collisions are emulated by equal hashes of unequal rows via a constant
    column layout)."""
    import torch
    from qpgesture_amd.sorted_rows import SortedRows
    torch.manual_seed(0)
    n, d = 300, 16
    x = torch.randn(n, d)
    codes = torch.randint(0, 5, (n,))
    x[10], codes[10] = x[3], codes[3]
    x[50], codes[50] = x[3], (codes[3] + 1) % 5             # same row, OTHER code: kept
    x[51], codes[51] = x[7], codes[7]
    x[120], codes[120] = x[119], codes[119]
    x[200], codes[200] = x[10], codes[10]                   # third copy
    keep = torch.tensor([i for i in range(n) if i != 119])  # 119 masked out: 120 is then the first of its kind
    m = SortedRows._first_of_duplicates(x, codes, keep)
    dropped = keep[~m].tolist()
    assert dropped == [10, 51, 200]
    # -0.0 and +0.0 are the same number: rows differing only there are duplicates
    y = torch.zeros(4, 8)
    y[1, 3] = -0.0
    y[2, 5] = 1.0
    m = SortedRows._first_of_duplicates(y, torch.zeros(4, dtype=torch.int64), torch.arange(4))
    assert m.tolist() in ([True, False, True, False], [True, True, True, False])   # (a -0.0 row may hash apart: kept)


def test_package_asks_for_device_kernargs_unless_the_user_chose():
    """qpgesture_amd/__init__.py: HIP_FORCE_DEV_KERNARG=1 by default (read by the HIP runtime at its initialisation), a
    value already in the environment is left alone."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import os; %s; import qpgesture_amd; print(os.environ['HIP_FORCE_DEV_KERNARG'])"
    for prelude, want in (("os.environ.pop('HIP_FORCE_DEV_KERNARG', None)", "1"),
                          ("os.environ['HIP_FORCE_DEV_KERNARG'] = '0'", "0")):
        r = subprocess.run([sys.executable, "-c", code % prelude], cwd=root, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip().splitlines()[-1] == want


def test_db_cache_file_format_roundtrip_on_the_host(tmp_path):
    """db_cache.py without a GPU: scalars, lists, nested dicts, NumPy arrays, host tensors, aliases and nested package
    objects survive save -> load bit for bit; a foreign key, a wrong magic and a short file are refused; the key follows
    the files' size / mtime and the options."""
    import torch
    from qpgesture_amd import db_cache
    from qpgesture_amd.code_knn import GestureDB
    from qpgesture_amd.sorted_rows import SortedRows
    db = object.__new__(GestureDB)
    sub = object.__new__(SortedRows)
    sub.__dict__.update(R=64, band=8.6e-5, row_code=torch.arange(64, dtype=torch.int16), device=torch.device("cpu"))
    t = torch.arange(12, dtype=torch.int32).reshape(3, 4)
    db.__dict__.update(N=7, feature_dtype="f16", aud_k=[0, 6, 12], shape=(2, 3), hl_bound_report={"kappa": 8.3, "families": {"a": [1.0, 2.0]}},
                       freq_dist=np.linspace(0, 1, 5), code_host=np.arange(6, dtype=np.int64).reshape(2, 3), txt_r=t, txt_cidx=t,
                       txt_sorted=sub, hl_image=None, device=torch.device("cpu"), flag=True, lo=np.int64(3))
    p = str(tmp_path / "x.qpgdb")
    db_cache.save(db, p, "kk")
    assert db_cache.load(p, "cpu", "other") is None
    got = db_cache.load(p, "cpu", "kk")
    assert type(got) is GestureDB and type(got.txt_sorted) is SortedRows
    assert got.N == 7 and got.feature_dtype == "f16" and got.aud_k == [0, 6, 12] and got.shape == (2, 3) and got.flag is True
    assert got.lo == 3 and got.hl_image is None and got.hl_bound_report == db.hl_bound_report
    assert got.freq_dist.dtype == np.float64 and np.array_equal(got.freq_dist, db.freq_dist)
    assert np.array_equal(got.code_host, db.code_host) and torch.equal(got.txt_r, t) and got.txt_cidx is got.txt_r
    assert torch.equal(got.txt_sorted.row_code, sub.row_code) and got.txt_sorted.band == 8.6e-5
    assert got.device == torch.device("cpu") and got.txt_sorted.device == torch.device("cpu")
    raw = open(p, "rb").read()
    open(p, "wb").write(b"NOTQPGDB" + raw[8:])
    assert db_cache.load(p, "cpu", "kk") is None
    open(p, "wb").write(raw[:-100])
    assert db_cache.load(p, "cpu", "kk") is None
    f1 = tmp_path / "a.npz"
    f1.write_bytes(b"123")
    k1 = db_cache.file_key([str(f1)], {"tie_rule": "numpy"})
    assert k1 == db_cache.file_key([str(f1)], {"tie_rule": "numpy"}) != db_cache.file_key([str(f1)], {"tie_rule": "stable"})
    os.utime(str(f1), ns=(5, 5))
    assert db_cache.file_key([str(f1)], {"tie_rule": "numpy"}) != k1
    # round 6: a header that names a foreign module / a non-class, or that does not parse, is a MISS - never an
    # import of that module and never an exception on every later run
    import json
    open(p, "wb").write(raw)
    hl = int.from_bytes(raw[8:16], "little")
    head = json.loads(raw[16:16 + hl].decode())

    for bad in (dict(head, **{"class": "os:system"}), dict(head, **{"class": "qpgesture_amd.db_cache:VERSION"}),
                dict(head, **{"class": "nonsense"}), dict(head, tensors=[{"name": "x"}]), dict(head, attrs=7),
                dict(head, data_bytes="many")):
        hb = json.dumps(bad).encode()
        if len(hb) > hl:
            continue
        blob = raw[:8] + hl.to_bytes(8, "little") + hb + b" " * (hl - len(hb)) + raw[16 + hl:]   # (JSON ignores the padding)
        open(p, "wb").write(blob)
        assert db_cache.load(p, "cpu", "kk") is None, bad
    nested = json.loads(json.dumps(head))
    nested["attrs"]["txt_sorted"]["__object__"] = "subprocess:Popen"
    hb = json.dumps(nested).encode()
    open(p, "wb").write(raw[:8] + hl.to_bytes(8, "little") + hb + b" " * (hl - len(hb)) + raw[16 + hl:])
    assert db_cache.load(p, "cpu", "kk") is None
    open(p, "wb").write(raw[:16] + b"{" * hl + raw[16 + hl:])
    assert db_cache.load(p, "cpu", "kk") is None
    # save(): a failure leaves no tmp file behind; eviction by sources and by count
    db.bad = torch.arange(12).reshape(3, 4).t()                        # not contiguous
    with pytest.raises(ValueError):
        db_cache.save(db, p, "kk")
    assert not [n for n in os.listdir(str(tmp_path)) if ".tmp." in n]
    del db.__dict__["bad"]
    d2 = tmp_path / "cache"
    paths = [str(d2 / ("db_%02d.qpgdb" % i)) for i in range(4)]
    db_cache.save(db, paths[0], "k0", sources="S")
    db_cache.save(db, paths[1], "k1", sources="T")
    db_cache.save(db, paths[2], "k2", sources="S")                     # same sources as [0]: [0] goes
    assert sorted(os.listdir(str(d2))) == ["db_01.qpgdb", "db_02.qpgdb"]
    db_cache.save(db, paths[3], "k3", sources="U", keep=2)             # at most two files stay: the oldest ([1]) goes
    assert sorted(os.listdir(str(d2))) == ["db_02.qpgdb", "db_03.qpgdb"]
    assert db_cache.load(paths[3], "cpu", "k3") is not None


def test_c_abi_argument_checks_under_asan_ubsan():
    """the host side of the C ABI - argument checks, size computations, error formatting - built with
    AddressSanitizer + UndefinedBehaviorSanitizer (python -m qpgesture_amd.build --sanitize) and driven by
    tools/abi_sanitize.py: every entry point refuses null / zero / negative / huge arguments with an error code and a
    message, the size helpers survive the edges of their integer ranges, and neither sanitizer reports anything."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "abi_sanitize.py")], capture_output=True, text=True,
                       timeout=1200)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "no sanitizer report" in r.stdout and "refused with a message" in r.stdout


def test_bench_sub_records_commands_parse():
    """bench.py's `sub_records` (round 6: BASELINE configs[2], [3] on one GPU, [4] in the driver's own line) are this script run
    again with other flags: every command must parse, must not recurse into further sub-records, and must name the
    configuration it claims."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(root, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    got = {}
    for name, what, flags in b.SUB_RUNS:
        a = b.build_parser().parse_args(flags + b.SUB_COMMON)
        assert a.no_sub_records and a.gpus == 1 and a.no_cpu_baseline and a.steps >= 20 and what
        assert a.full                  # (the records read the child's --full fields: eager leg, graph replay check, ...)
        got[name] = a
    assert got["cfg3"].workload == "cfg3"
    assert got["strong8192"].scaling == "strong" and got["strong8192"].n_db is None        # (strong: 8192 windows)
    c = got["clips16_f16_enc96"]
    assert (c.clips, c.feature_dtype, c.encode_batch, c.encode_precision) == (16, "f16", 96, "f32")
    assert got["clips16_f16_enc96_f16x3"].encode_precision == "f16x3"
    d = b.build_parser().parse_args([])                                                     # the driver's default run
    assert not d.no_sub_records and d.gpus == 1 and d.workload == "match"
    assert not d.full and d.dump_outputs is None                                            # (a plain run: headline only)


def test_bench_dump_outputs_writes_float64(tmp_path):
    """bench.py --dump-outputs: every array as <DIR>/<name>.npy in float64 (integer codes exact), one file per rank with
    N > 1 ranks, and no more than 64 MB in all."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(root, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    codes = np.arange(180, dtype=np.int32).reshape(6, 30) * 3
    b.dump_outputs(str(tmp_path / "one"), {"codes": codes}, 1, 0)
    got = np.load(tmp_path / "one" / "codes.npy")
    assert got.dtype == np.float64 and np.array_equal(got, codes)
    b.dump_outputs(str(tmp_path / "two"), {"codes": codes}, 2, 1)
    assert os.listdir(tmp_path / "two") == ["codes_rank1.npy"]
    with pytest.raises(ValueError):
        b.dump_outputs(str(tmp_path / "big"), {"x": np.zeros((b.DUMP_LIMIT_BYTES // 8 + 1,), np.float32)}, 1, 0)


# ---- the step plan (code_knn.plan_audio / plan_text / plan_step): which kernels a call takes, decided on plain values ----
_HL, _MX = ck.AUDIO_HL_BAND, ck.AUDIO_MX_BAND
_ONE_GPU = dict(n_local=2048, N=2048, world=1, K=512, Ga=26, F=1024, Dt=384)
_SHARD = dict(_ONE_GPU, n_local=1024, world=2)            # one of two row shards


def _step(db=_ONE_GPU, M=3, steps=8, mode=ck.MODE_AUD_TXT, for_walk=True, owner_blocks=False, **knobs):
    p = ck.plan_step(ck.Knobs(**knobs), ck.DBFacts(**db), M, steps, mode, for_walk, owner_blocks)
    return (None if p.audio is None else tuple(p.audio),) + tuple(p[1:])


def test_step_plan_table():
    """A literal table of plans, written from the conditions of the kernels' paths (not produced by the functions):
    (audio = (path, sweep kernel, band, cut, ranks fused) | None, text, sharded, exchange, one-launch pack, split rank
    fusion, overlap, order)."""
    hl1 = ("mixed", "hl", _HL, 1, True)
    f16 = dict(_ONE_GPU, feature_dtype="f16", hl_planes=1)
    table = [
        # a one-GPU default clip into the walk; the same with return_tables (no cut, no split fusion)
        (dict(), (hl1, "mfma", False, None, True, True, True, "audio_first")),
        (dict(for_walk=False), (("mixed", "hl", _HL, 0, True), "mfma", False, None, True, False, True, "audio_first")),
        (dict(mode=ck.MODE_AUD), (("mixed", "hl", _HL, 2, True), None, False, None, False, False, False, None)),
        (dict(mode=ck.MODE_TXT), (None, "mfma", False, None, False, False, False, None)),
        # each knob alone
        (dict(audio_precision="f64"), (("guarded", "f64", 0.0, 0, True), "mfma", False, None, False, True, True, "audio_first")),
        (dict(audio_precision="exact"),
         (("exact", "f64", 0.0, 0, True), "valu", False, None, False, True, True, "text_after_sweep")),
        (dict(audio_kernel="mx"), (("mixed", "mx", _MX, 1, True), "mfma", False, None, False, True, True, "audio_first")),
        (dict(text_kernel="valu"), (hl1, "valu", False, None, False, True, True, "text_after_sweep")),
        (dict(fused_pack=False), (hl1, "mfma", False, None, False, True, True, "audio_first")),
        (dict(split_fuse=False), (hl1, "mfma", False, None, True, False, True, "audio_first")),
        (dict(rank_cut=False), (("mixed", "hl", _HL, 0, True), "mfma", False, None, True, True, True, "audio_first")),
        (dict(mixed_single_launch=True), (("mixed", "hl", _HL, 0, True), "mfma", False, None, True, True, True, "audio_first")),
        (dict(tie_eps=0.0), (("plain", "f64", 0.0, 0, True), "mfma", False, None, False, True, True, "audio_first")),
        (dict(host_ranks=True), (("mixed", "hl", _HL, 0, True), "mfma", False, None, True, False, True, "audio_first")),
        # the five schedules of test_knn_pred_vs_reference_golden: auto, text_after_sweep, text_first, audio_first, one_stream
        (dict(audio_first=None), (hl1, "mfma", False, None, True, True, True, "audio_first")),
        (dict(text_after_sweep=True, audio_first=False), (hl1, "mfma", False, None, True, True, True, "text_after_sweep")),
        (dict(text_after_sweep=False, audio_first=False), (hl1, "mfma", False, None, True, True, True, "text_first")),
        (dict(text_after_sweep=False, audio_first=True), (hl1, "mfma", False, None, True, True, True, "audio_first")),
        (dict(overlap_sweeps=False), (hl1, "mfma", False, None, False, True, False, None)),
        # facts of the database
        (dict(db=f16), (("mixed", "hl1", _HL, 1, True), "mfma", False, None, True, True, True, "audio_first")),
        (dict(db=f16, audio_kernel="mx"), (("mixed", "mx_h", _MX, 1, True), "mfma", False, None, False, True, True, "audio_first")),
        (dict(db=f16, audio_precision="f64"),
         (("guarded", "f64_h", 0.0, 0, True), "mfma", False, None, False, True, True, "audio_first")),
        (dict(db=dict(_ONE_GPU, hl_bound_ok=False)),
         (("guarded", "f64", 0.0, 0, True), "mfma", False, None, False, True, True, "audio_first")),
        (dict(db=dict(_ONE_GPU, hl_bound_ok=False, has_hl_image=False, has_txt_sorted=False)),   # as GestureDB leaves it
         (("guarded", "f64", 0.0, 0, True), "valu", False, None, False, True, True, "text_after_sweep")),
        (dict(db=dict(_ONE_GPU, has_hl_image=False)),
         (("mixed", "mx", _MX, 1, True), "mfma", False, None, False, True, True, "audio_first")),
        (dict(db=dict(_ONE_GPU, K=1024)), (("guarded", "f64", 0.0, 0, True), "mfma", False, None, False, True, True, "audio_first")),
        (dict(db=dict(_ONE_GPU, K=520)), (("guarded", "f64", 0.0, 0, True), "mfma", False, None, False, False, True, "audio_first")),
        (dict(db=dict(_ONE_GPU, Dt=320)), (hl1, "mfma", False, None, False, True, True, "audio_first")),
        (dict(db=dict(_SHARD, n_local=0, has_hl_image=False, has_txt_sorted=False)),              # an empty shard
         (("plain", "f64", 0.0, 0, False), "valu", True, "all_gather", False, False, True, "text_after_sweep")),
        # the wavvq sweep has one path, takes no pack and is never waited for by the text side
        (dict(use_wavvq=True), (None, "mfma", False, None, False, True, True, "audio_first")),
        (dict(use_wavvq=True, text_after_sweep=True, audio_first=False), (None, "mfma", False, None, False, True, True, "text_first")),
        # split fusion up to split_fuse_max_steps = 256 steps: 32 x 8 = 256, 33 x 8 = 264
        (dict(M=32), (hl1, "mfma", False, None, True, True, True, "audio_first")),
        (dict(M=33), (hl1, "mfma", False, None, True, False, True, "audio_first")),
        # row shards: 2e-9 * Q * 1024 * 26 * 6 * 1024 GFLOP per rank = 7.85 (Q = 24), 31.4 (Q = 96) against 20
        (dict(db=_SHARD), (("guarded", "f64", 0.0, 0, False), "mfma", True, "all_gather", False, False, True, "audio_first")),
        (dict(db=_SHARD, M=12), (("mixed", "hl", _HL, 0, False), "mfma", True, "all_gather", True, False, True, "audio_first")),
        (dict(db=_SHARD, M=12, owner_blocks=True),
         (("mixed", "hl", _HL, 0, False), "mfma", True, "all_to_all", True, False, True, "audio_first")),
        (dict(db=_SHARD, M=12, sharded_mixed=False),
         (("guarded", "f64", 0.0, 0, False), "mfma", True, "all_gather", False, False, True, "audio_first")),
        (dict(db=_SHARD, M=12, audio_kernel="mx"),
         (("mixed", "mx", _MX, 0, False), "mfma", True, "all_gather", False, False, True, "audio_first")),
        (dict(db=_SHARD, M=12, audio_precision="exact", owner_blocks=True),
         (("exact", "f64", 0.0, 0, False), "valu", True, "all_to_all", False, False, True, "text_after_sweep")),
        # force_sharded on one GPU: 2e-9 * 24 * 2048 * 26 * 6 * 1024 = 15.7 GFLOP
        (dict(force_sharded=True), (("guarded", "f64", 0.0, 0, False), "mfma", True, "all_gather", False, False, True, "audio_first")),
        (dict(force_sharded=True, sharded_mixed_min_gflop=0.0, owner_blocks=True),
         (("mixed", "hl", _HL, 0, False), "mfma", True, "all_to_all", True, False, True, "audio_first")),
        (dict(force_sharded=True, mode=ck.MODE_AUD, sharded_mixed_min_gflop=0.0),
         (("mixed", "hl", _HL, 0, False), None, True, "all_gather", False, False, False, None)),
    ]
    for kw, want in table:
        assert _step(**kw) == want, kw
    # the stand-alone sweeps (search_*_cands, tests): no ranks wanted -> nothing fused, the f64 sweep + guard
    kn, db = ck.Knobs(), ck.DBFacts(**_ONE_GPU)
    assert tuple(ck.plan_audio(kn, db, 1)) == ("guarded", "f64", 0.0, 0, False)
    assert tuple(ck.plan_audio(kn, db, 24, want_rank=True, cut_top_n=2)) == ("mixed", "hl", _HL, 2, True)
    assert tuple(ck.plan_audio(kn, db, 24, want_rank=True, cut_top_n=3)) == ("mixed", "hl", _HL, 0, True)
    assert ck.plan_text(kn, db, 1) == "mfma" and ck.plan_text(kn, db, 0) == "valu"
    assert ck.plan_text(kn, db, 1, reduce=False) == "valu" and ck.plan_text(kn, db, 1, reduce=False, out_given=True) == "mfma"
    assert ck.plan_text(kn, ck.DBFacts(**_SHARD), 1) == "valu"


def test_step_plan_hands_each_side_its_own_plan():
    """For every combination of the boolean knobs, the audio / text parts of the step's plan are what plan_audio /
    plan_text give for the arguments sweep_tables passes to the two sides - and the one-launch pack is only planned
    where the audio side takes the split-f16 sweep and the text side the prefilter that read the pack's images."""
    import itertools
    bools = ["overlap_sweeps", "text_after_sweep", "fused_pack", "rank_cut", "split_fuse", "host_ranks", "use_wavvq",
             "force_sharded", "sharded_mixed", "mixed_single_launch"]
    n = 0
    for vals in itertools.product((False, True), repeat=len(bools)):
        for prec, af, db, for_walk in itertools.product(("mixed", "exact"), (None, False), (_ONE_GPU, _SHARD), (False, True)):
            kn = ck.Knobs(audio_precision=prec, audio_first=af, sharded_mixed_min_gflop=0.0, **dict(zip(bools, vals)))
            facts = ck.DBFacts(**db)
            sharded = facts.world > 1 or kn.force_sharded
            for mode in (ck.MODE_AUD_TXT, ck.MODE_AUD, ck.MODE_TXT):
                p = ck.plan_step(kn, facts, 3, 8, mode, for_walk)
                cut = 0
                if for_walk and kn.rank_cut and not sharded and not kn.use_wavvq and not kn.host_ranks:
                    cut = 1 if mode == ck.MODE_AUD_TXT else 2
                want_a = None if (mode == ck.MODE_TXT or kn.use_wavvq) else ck.plan_audio(
                    kn, facts, 24, want_rank=not sharded, reduce=not sharded, out_given=sharded, cut_top_n=cut)
                want_t = None if mode == ck.MODE_AUD else ck.plan_text(kn, facts, 24, reduce=not sharded, out_given=sharded)
                assert p.audio == want_a and p.text == want_t and p.sharded == sharded
                assert p.overlap == (p.order is not None) == (mode == ck.MODE_AUD_TXT and kn.overlap_sweeps)
                if p.clip_pack:
                    assert p.audio.kernel == "hl" and p.text == "mfma" and p.overlap
                n += 1
    assert n == 2 ** len(bools) * 16 * 3


def test_matcher_declares_its_state_and_its_knobs_feed_the_plan():
    """CodeKNN hands the plan functions its own knobs, field by field, with the defaults Knobs() states; every member
    it uses exists after __init__ (no member appears on first use), and no method decides by a `_last_*` diagnostic."""
    import re
    import types
    import torch
    fake = types.SimpleNamespace(step_sz=6, T=180, N=4, device=torch.device("cpu"), n_local=4, world=1, K=512, Ga=26, F=8,
                                 Dt=384, feature_dtype="f32", hl_bound_ok=True, hl_image=None, txt_sorted=object(), hl_planes=2)
    knn = ck.CodeKNN(fake)
    if "QPG_FUSED_PACK" not in os.environ and "QPG_RANK_CUT" not in os.environ:
        assert knn._knobs() == ck.Knobs()
    for i, f in enumerate(ck.Knobs._fields):
        setattr(knn, f, "knob%d" % i)
    assert knn._knobs() == ck.Knobs(*["knob%d" % i for i in range(len(ck.Knobs._fields))])
    assert knn._facts() == ck.DBFacts(4, 4, 1, 512, 26, 8, 384, "f32", True, False, True, 2)
    src = open(ck.__file__).read()
    body = src[src.index("class CodeKNN"):]
    assert "self.__dict__" not in body and "getattr(self," not in body
    for gone in ("_hl_plan", "_want_sweep_event", "_sweep_done"):
        assert gone not in src
    used = set(re.findall(r"self\.(_?[a-z]\w*)\b(?!\()", body))
    methods = set(re.findall(r"def (\w+)\(", body))
    assert not {u for u in used if u not in methods and not hasattr(knn, u)}
    reads = [l.strip() for l in body.splitlines() if "self._last_" in l.rsplit(" = ", 1)[-1]]
    assert reads == ["ws, Q = self._mix_ws, self._last_mix_Q"]          # (tier1_list_lengths: itself a diagnostic)
