"""2-D train-step time of the reference's training example (EM2EM(132, is3d=False)) at batch 64 and batch 1, fp32 and bf16,
measured alternately in one process with device events: 20 warm-up steps per case, then rounds of --chunk timed steps
per case until each case has --steps.  Prints one JSON line: ms/step and steps/s per case.

    python tests/tools/step2d_time.py [--steps 100] [--chunk 10] [--warmup 20]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from transfer_em_amd.cgan import EM2EM  # noqa: E402


def _inputs(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, shape, dtype=np.uint8).astype(np.float32) / np.float32(127.5) - np.float32(1.0)
    return torch.from_numpy(((x - x.mean()) / x.std()).astype(np.float32)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        for batch in (64, 1):
            for prec in ("fp32", "bf16"):
                tag = f"{prec}_b{batch}"
                model = EM2EM(132, tag, is3d=False, checkpoint_root=tmp, precision=prec)
                shape = (batch, 1, 132, 132, 1)
                cases[tag] = dict(model=model, rx=_inputs(shape, 1), ry=_inputs(shape, 2), ms=0.0, n=0)
        for c in cases.values():
            for _ in range(args.warmup):
                c["model"].train_step(c["rx"], c["ry"])
        torch.cuda.synchronize()
        while any(c["n"] < args.steps for c in cases.values()):
            for c in cases.values():
                if c["n"] >= args.steps:
                    continue
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.chunk):
                    c["model"].train_step(c["rx"], c["ry"])
                b.record()
                b.synchronize()
                c["ms"] += a.elapsed_time(b)
                c["n"] += args.chunk
        out = {"workload": "EM2EM(132, is3d=False).train_step", "warmup": args.warmup}
        for tag, c in cases.items():
            ms = c["ms"] / c["n"]
            out[tag] = dict(ms_per_step=round(ms, 4), steps_per_s=round(1e3 / ms, 2), timed_steps=c["n"])
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
