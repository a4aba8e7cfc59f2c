"""The gfx950 code of every kernel of a tree, as hashes: something to compare two trees with.

    python tools/kernel_asm_hash.py ROOT [--host] [--keep DIR] > a.jsonl     # one JSON line per csrc/*.hip of ROOT
    python tools/kernel_asm_hash.py --diff a.jsonl b.jsonl                   # exit status 1 unless every hash is equal

Every source is compiled with ROOT's own build.FLAGS (minus -shared) plus `-cuid=qpg --offload-device-only -S`; the line
of a source is {"source": name, "kernels": {kernel symbol: sha256}}.  The hashed text of a kernel runs from its label to
its .Lfunc_end marker, followed by its .amdhsa_kernel ... .end_amdhsa_kernel block.  Two things are taken out first: the
ordinal that the compiler gives a function inside its file (.LBB<n>_<m>, .Lfunc_end<n>), which shifts for every kernel
behind one that was removed, and the assembly's comments, which repeat it ("Header=BB<n>_<m>").  --host compiles with
--offload-host-only -S instead and hashes the whole file ({"source", "host"}); --keep leaves the assembly in DIR for diff.
A change that must leave the generated code alone (a removed build knob, a moved comment) is checked by running this on
the parent's tree and on the new one; the tool reads nothing but the compiler's output."""
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

JOBS = 16


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def kernel_hashes(asm):
    asm = re.sub(r"[ \t]*;.*", "", asm)
    asm = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+", r".\1", asm)
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel\n", asm, re.M | re.S):
        name = m.group(1)
        body = re.search(r"^%s:.*?^\.Lfunc_end:\n" % re.escape(name), asm, re.M | re.S)
        out[name] = sha(body.group(0) + m.group(0))
    return out


def compile_tree(root, host, keep):
    spec = importlib.util.spec_from_file_location("qpg_build", os.path.join(root, "qpgesture_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    mode = "--offload-host-only" if host else "--offload-device-only"
    flags = [f for f in build.FLAGS if f != "-shared"] + ["-cuid=qpg", mode, "-S"]

    def one(src):
        name = os.path.basename(src)
        out = os.path.join(keep, name[:-4] + (".host.s" if host else ".s"))
        subprocess.check_call([build.HIPCC] + flags + [name, "-o", out], cwd=os.path.dirname(src))
        with open(out) as f:
            asm = f.read()
        return {"source": name, "host": sha(asm)} if host else {"source": name, "kernels": kernel_hashes(asm)}

    with ThreadPoolExecutor(min(JOBS, os.cpu_count() or 1)) as pool:
        for line in pool.map(one, build.sources()):
            print(json.dumps(line, sort_keys=True), flush=True)


def diff(pa, pb):
    def load(p):
        with open(p) as f:
            return {d["source"]: d.get("kernels", {"<host>": d.get("host")}) for d in map(json.loads, f)}
    a, b = load(pa), load(pb)
    bad = 0
    for src in sorted(set(a) | set(b)):
        ka, kb = a.get(src, {}), b.get(src, {})
        differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
        gone, new = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
        print("%-22s %3d / %3d symbols  %s" % (src, len(ka), len(kb), "DIFFER" if differ or gone or new else "all equal"))
        for tag, names in (("differs", differ), ("vanished", gone), ("new", new)):
            for k in names:
                print("   %-9s %s" % (tag, k))
        bad += len(differ) + len(gone) + len(new)
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) == 3 and args[0] == "--diff":
        sys.exit(diff(args[1], args[2]))
    host = "--host" in args
    keep = args[args.index("--keep") + 1] if "--keep" in args else None
    root = os.path.abspath(args[0])
    if keep:
        os.makedirs(keep, exist_ok=True)
        compile_tree(root, host, os.path.abspath(keep))
    else:
        with tempfile.TemporaryDirectory() as tmp:
            compile_tree(root, host, tmp)
