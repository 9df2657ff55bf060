"""Writes tests/golden/perspective_torch_cpu.json: for each seeded perspective case, the coefficients torch's own
least squares gives (torchvision _get_perspective_coeffs) and the sha256 of torchvision's tensor-path perspective run on
torch's CPU primitives (tests/tv_perspective_ref.py), the arithmetic the reference's apply_perspective_warp
(fall_2025/transformations_code:54-66) ends up in.  The contraction and accumulation order of those primitives depends
on the CPU kernels a torch build dispatches to, so the outputs are recorded once with the build the oracle was pinned
to and the test compares the oracle with the record.
usage: python tests/golden/make_perspective_golden.py"""
import hashlib, json, os, sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import imgxf_oracle as O  # noqa: E402


def cases():
    """(trial, w, h, startpoints, endpoints): 24 sizes and distortion scales, the endpoints drawn the way
    RandomPerspective draws them from a seeded torch generator."""
    rng = np.random.default_rng(11)
    for trial in range(24):
        w, h = int(rng.integers(8, 160)), int(rng.integers(8, 160))
        g = torch.Generator().manual_seed(trial)
        ds = (0.0, 0.05, 0.1, 0.2, 0.5, 0.9)[trial % 6]
        st, en = O.perspective_endpoints(w, h, ds, lambda lo, hi: int(torch.randint(lo, hi, size=(1,), generator=g).item()))
        yield trial, w, h, st, en


def image(trial, h, w, ch):
    """uint8 HxWxch input (HxW for ch == 1), default_rng(100 + trial).integers(0, 256, ...)."""
    rng = np.random.default_rng(100 + trial)
    if ch == 1:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)[..., 0].copy()
    return rng.integers(0, 256, (h, w, ch), dtype=np.uint8)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import tv_perspective_ref as TV
    rows = []
    for trial, w, h, st, en in cases():
        c = TV.coeffs(st, en)
        for ch in (3, 1, 4):
            rows.append({"trial": trial, "w": w, "h": h, "ch": ch, "coeffs": c,
                         "sha256": sha256(TV.perspective_u8(image(trial, h, w, ch), c))})
    with open(os.path.join(HERE, "perspective_torch_cpu.json"), "w") as f:
        json.dump({"torch": torch.__version__, "cases": rows}, f, indent=1)
    print(len(rows), "cases")
