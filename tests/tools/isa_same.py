"""Device code of two source trees compared, file by file: python tests/tools/isa_same.py TREE_A TREE_B [file.hip ...]
Every csrc/*.hip of both trees is compiled with build.py's FLAGS plus `--cuda-device-only -S` (as isa_mix.py does).
Comments, directives, local labels and the __hip_cuid_ label are dropped; what remains -- kernel labels and
instructions -- must be byte-identical, and so must every kernel's register counts, scratch / LDS size and
kernel-argument size.  The check of a host-side refactor: exit status 1 if any file differs."""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from transfer_em_amd.build import FLAGS, HIPCC
META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size")


def device_code(tree, f, tmp):
    src = os.path.join(tree, "transfer_em_amd", "csrc", f)
    if not os.path.exists(src):
        return None
    out = os.path.join(tmp, f"{abs(hash(tree))}_{f}.s")
    subprocess.run([HIPCC] + FLAGS + ["--cuda-device-only", "-S", "-o", out, src], stderr=subprocess.DEVNULL, check=True)
    text, meta = [], []
    for l in open(out):
        s = l.strip()
        if s.startswith(".name:") or s.startswith(META):
            meta.append(s)
        if not s or s[0] in ";." or "__hip_cuid_" in s:
            continue
        text.append(re.sub(r"\s*;.*$", "", l.rstrip()))
    return text, meta


def main():
    a, b = sys.argv[1:3]
    csrc = [os.path.join(t, "transfer_em_amd", "csrc") for t in (a, b)]
    files = sys.argv[3:] or sorted({f for d in csrc for f in os.listdir(d) if f.endswith(".hip")})
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        jobs = [(f, ex.submit(device_code, a, f, tmp), ex.submit(device_code, b, f, tmp)) for f in files]
        for f, ja, jb in jobs:
            ra, rb = ja.result(), jb.result()
            if ra is None or rb is None:
                verdict = "only in one tree"
            elif ra[0] != rb[0]:
                verdict = f"instructions differ ({sum(x != y for x, y in zip(ra[0], rb[0])) + abs(len(ra[0]) - len(rb[0]))} lines)"
            elif ra[1] != rb[1]:
                verdict = "kernel metadata differs"
            else:
                verdict = None
            bad += verdict is not None
            print(f"{f:24s} {verdict or 'same'}" + (f"  ({len(ra[0])} lines, {sum(m.startswith('.vgpr_count') for m in ra[1])} kernels)" if ra and not verdict else ""), flush=True)
    print(f"{len(files) - bad} of {len(files)} files have identical device code")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
