"""Whole-call times of the seven list passes on the 1024-frame, 343-size set of tools/bench_preprocess_list.py (256 of
its frames for `apply_chain_list`), one JSON line per pass with every repeat and a digest of the outputs.  `--root DIR`
imports the package from another checkout (IMGXF_LIBRARY names the library where that checkout has none built), so the
same script times a parent commit: run the two alternately, process by process, and hold the candidate against the
parent's own run-to-run spread (profiles/list_block.txt).  Needs a ROCm device.

    python tools/bench_list_passes.py --root . --label candidate [--repeats 7] [--frames 1024]
"""
import argparse, hashlib, json, os, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--root", required=True)
ap.add_argument("--label", required=True)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--frames", type=int, default=1024)
args = ap.parse_args()
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(args.root))
sys.path.insert(0, HERE)
import numpy as np
import torch
import imagetransformations_amd as pkg
assert os.path.abspath(pkg.__file__).startswith(os.path.abspath(args.root)), pkg.__file__
from imagetransformations_amd import tensor_maps as M, resize_list as RL, driver_list as DL, pool as P, jpeg as J
from bench_preprocess_list import mixed_sizes, noise_frames, MEAN, STD
import random

dev = torch.device("cuda:0")
sizes = mixed_sizes(args.frames)
frames, _ = noise_frames(sizes, dev, 1)
torch.manual_seed(0)
boxes, flips = M.random_resized_crop_params(sizes)
targets = RL.shorter_side_sizes(sizes, 256)
entries = [(i, name, (v,)) for i in range(len(frames)) for name, v in (("scale", 1.1), ("lighten_darken", 0.2), ("contrast", 1.2))]
chain = ["defocus_blur", "enhance_contrast", "motion_blur"]
few = frames[:256]


def digest(out):
    h = hashlib.sha256()
    if isinstance(out, torch.Tensor):
        out = [out]
    if isinstance(out, tuple):
        out = [o for o in out[0] if o is not None]
    for o in out:
        h.update(o.cpu().numpy().tobytes() if isinstance(o, torch.Tensor) else bytes(o))
    return h.hexdigest()[:16]


def chain_call():
    random.seed(3); np.random.seed(3)
    return P.apply_chain_list(few, chain)


WORK = {
    "preprocess_list": lambda: M.preprocess_list(frames, 256, 224, MEAN, STD),
    "resized_crop_list": lambda: M.resized_crop_list(frames, boxes, 224, flips, mean=MEAN, std=STD),
    "resize_list": lambda: RL.resize_list(frames, targets),
    "apply_list": lambda: DL.apply_list(frames, entries),
    "apply_chain_list_256": chain_call,
    "encode_list_views": lambda: J.encode_list_views(frames, 75),
    "roundtrip_list": lambda: J.roundtrip_list(frames, 75),
}
for name, fn in WORK.items():
    out = fn()                                               # warm-up; its result is the digest
    torch.cuda.synchronize()
    d = digest(out)
    del out
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        del out
    print(json.dumps({"label": args.label, "work": name, "ms": [round(t, 3) for t in times], "digest": d}), flush=True)
