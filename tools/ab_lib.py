"""Same-process A/B of two builds of libimgxf.so on the headline kernels (development aid).

    python tools/ab_lib.py <libA.so> <libB.so> [affine|affine32|gaussian|nearest|all|step|pixel] [frames] [height width]

(frames of 2160 x 3840 unless a height and a width are given: 128 x 2160 x 4096 is the width whose 32 tile columns
divide over the XCDs, 288 x 1440 x 2560 and 1152 x 720 x 1280 hold the bytes of 128 4K frames)

Both libraries are loaded with ctypes next to each other; the same C-ABI call on the same resident
frames is timed with HIP events, alternating A / B for ROUNDS rounds of ITERS launches, and the medians are
printed (box-to-box and process-to-process differences cancel).  Outputs are compared byte for byte."""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
from imagetransformations_amd import _ffi, ops  # noqa: E402

ROUNDS, ITERS = int(os.environ.get("ROUNDS", "7")), int(os.environ.get("ITERS", "8"))


def load(path, env=None, copy=False):
    """env: "NAME=value,NAME2=value" knobs that only THIS library instance sees (every copy of libimgxf.so caches its own
    knob table: the variables are set, the library re-reads them, they are removed again).  copy: a second instance of a
    library that is already loaded."""
    if env or copy:
        import shutil, tempfile
        tmp = tempfile.NamedTemporaryFile(suffix=".so", delete=False).name       # a second dlopen of one path is the same instance
        shutil.copy(path, tmp)
        path = tmp
    lib = C.CDLL(path)
    if env:
        pairs = [kv.split("=", 1) for kv in env.split(",")]
        for k, v in pairs: os.environ[k] = v
        lib.imgxf_reload_knobs()
        for k, _ in pairs: os.environ.pop(k)
    for name, argtypes in _ffi.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = C.c_int, argtypes
    return lib


def pixel(libs, src, st):
    """The per-pixel kernels that move a lane's chunk through load_chunk / store_chunk (csrc/imgxf_common.h) and
    imgxf_enhance_contrast_u8, on library A, a SECOND load of library A and library B, alternating.  A against A2 is the
    margin: B is slow where its median lies above both of theirs."""
    F, H, W, _ = src.shape
    src2 = src.flip(0).contiguous()
    rgb = {k: torch.empty_like(src) for k in libs}
    gray = {k: torch.empty((F, H, W, 1), dtype=torch.uint8, device=src.device) for k in libs}
    sums = torch.empty(F, dtype=torch.int64, device=src.device)
    vs, vs2 = _ffi.view_of(src), _ffi.view_of(src2)
    cases = {
        "scale_abs": (rgb, lambda lib, vo: lib.imgxf_scale_abs_u8(_ffi.vp(vs), _ffi.vp(vo), 1.5, 10.0, st), 6),
        "blend": (rgb, lambda lib, vo: lib.imgxf_blend_u8(_ffi.vp(vs), None, _ffi.vp(vs2), None, _ffi.vp(vo), 0.3, st), 9),
        "rgb2l": (gray, lambda lib, vo: lib.imgxf_rgb2l_u8(_ffi.vp(vs), _ffi.vp(vo), st), 4),
        "enhance_color": (rgb, lambda lib, vo: lib.imgxf_enhance_color_u8(_ffi.vp(vs), _ffi.vp(vo), 1.5, st), 6),
        "enhance_contrast": (rgb, lambda lib, vo: lib.imgxf_enhance_contrast_u8(_ffi.vp(vs), _ffi.vp(vo), 1.5, sums.data_ptr(), st), 9),
        "rgb2yuv": (rgb, lambda lib, vo: lib.imgxf_rgb2yuv_u8(_ffi.vp(vs), _ffi.vp(vo), st), 6),
    }
    px = F * H * W
    print(f"F={F} {H}x{W}x3, {ROUNDS} rounds of {ITERS} launches, medians in ms (GB/s); A2 = library A loaded a second time")
    for name, (outs, call, bpp) in cases.items():
        views = {k: _ffi.view_of(outs[k]) for k in libs}
        for k, lib in libs.items():
            outs[k].fill_(0x5a)
            rc = call(lib, views[k])
            assert rc == 0, (name, k, rc)
        torch.cuda.synchronize()
        equal = bool(torch.equal(outs["A"], outs["B"])) and bool(torch.equal(outs["A"], outs["A2"]))
        res = {k: [] for k in libs}
        order = list(libs)
        for rnd in range(ROUNDS):
            # the order rotates: the library that ran last in every round measured 2 % slow on IDENTICAL device code
            for k in order[rnd % 3:] + order[:rnd % 3]:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                call(libs[k], views[k]); s.record()
                for _ in range(ITERS):
                    call(libs[k], views[k])
                e.record(); torch.cuda.synchronize()
                res[k].append(s.elapsed_time(e) / ITERS)
        med = {k: statistics.median(v) for k, v in res.items()}
        slow = med["B"] > max(med["A"], med["A2"])
        print(f"{name:17s}" + "".join(f" {k} {med[k]:7.4f} ({bpp * px / med[k] / 1e6:5.0f})" for k in libs) +
              f"   B/A {med['B'] / med['A']:.4f}  A2/A {med['A2'] / med['A']:.4f}   B rounds {min(res['B']):.4f} .. {max(res['B']):.4f}"
              f"   {'SLOWER than both loads of A' if slow else 'inside'}   outputs equal: {equal}", flush=True)


def main():
    pa, pb = sys.argv[1], sys.argv[2]
    what = sys.argv[3] if len(sys.argv) > 3 else "all"
    F = int(sys.argv[4]) if len(sys.argv) > 4 else 128
    libs = {"A": load(pa, os.environ.get("A_ENV")), "B": load(pb, os.environ.get("B_ENV"))}
    H, W = (int(sys.argv[5]), int(sys.argv[6])) if len(sys.argv) > 6 else (2160, 3840)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    src = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    st = torch.cuda.current_stream().cuda_stream
    if what == "pixel":
        return pixel({"A": libs["A"], "A2": load(pa, os.environ.get("A_ENV"), copy=True), "B": libs["B"]}, src, st)
    outs = {k: torch.empty_like(src) for k in libs}
    vs = _ffi.view_of(src)
    m = _ffi.f64_array(ops.rotate_zoom_matrix(W, H, 30.0, 1.5))
    mn = _ffi.f64_array(ops.rotate_matrix(W, H, 22.5))
    fill = _ffi.u8_array([0, 0, 0])
    cases = {
        "affine": (lambda lib, vo: lib.imgxf_affine_u8(_ffi.vp(vs), _ffi.vp(vo), m, 1, fill, 1, None, st), 4.306),
        "affine32": (lambda lib, vo: lib.imgxf_affine_u8(_ffi.vp(vs), _ffi.vp(vo), m, 1, fill, 0, None, st), 4.306),
        "gaussian": (lambda lib, vo: lib.imgxf_gaussian_u8(_ffi.vp(vs), _ffi.vp(vo), 5, 5.0 / 6.0, None, st), 6.0),
        "nearest": (lambda lib, vo: lib.imgxf_affine_u8(_ffi.vp(vs), _ffi.vp(vo), mn, 0, fill, 1, None, st), 5.06),
        "gaussian31": (lambda lib, vo: lib.imgxf_gaussian_u8(_ffi.vp(vs), _ffi.vp(vo), 31, 5.0, None, st), 6.0),
    }
    if what == "step":
        # bench.py's step: Gaussian (src -> tmp) then rotate (tmp -> out), alternating libraries per round; per-kernel events
        tmp = torch.empty_like(src)
        vt = _ffi.view_of(tmp)
        res = {k: ([], []) for k in libs}
        for rnd in range(ROUNDS + 1):
            for k, lib in libs.items():
                vo = _ffi.view_of(outs[k])
                ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(ITERS)]
                for it in range(ITERS):
                    ev[it][0].record()
                    lib.imgxf_gaussian_u8(_ffi.vp(vs), _ffi.vp(vt), 5, 5.0 / 6.0, None, st)
                    ev[it][1].record()
                    lib.imgxf_affine_u8(_ffi.vp(vt), _ffi.vp(vo), m, 1, fill, 1, None, st)
                    ev[it][2].record()
                torch.cuda.synchronize()
                if rnd:
                    res[k][0].extend(e[0].elapsed_time(e[1]) for e in ev)
                    res[k][1].extend(e[1].elapsed_time(e[2]) for e in ev)
        px = F * H * W
        for k in libs:
            g, a = statistics.median(res[k][0]), statistics.median(res[k][1])
            print(f"step, library {k}: gaussian {g:7.4f} ms ({6.0 * px / g / 1e6 / 8000:.3f})  rotate {a:7.4f} ms ({4.306 * px / a / 1e6 / 8000:.3f})  "
                  f"step {g + a:7.4f} ms = {px / (g + a) / 1e3:9.1f} Mpix/s", flush=True)
        print("outputs equal:", bool(torch.equal(outs["A"], outs["B"])))
        return
    names = list(cases) if what == "all" else what.split(",")
    px = F * H * W
    for name in names:
        call, bpp = cases[name]
        res = {k: [] for k in libs}
        views = {k: _ffi.view_of(outs[k]) for k in libs}
        for k, lib in libs.items():
            rc = call(lib, views[k])
            assert rc == 0, (name, k, rc)
        torch.cuda.synchronize()
        equal = bool(torch.equal(outs["A"], outs["B"]))
        for _ in range(ROUNDS):
            for k, lib in libs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                call(lib, views[k]); s.record()
                for _ in range(ITERS):
                    call(lib, views[k])
                e.record(); torch.cuda.synchronize()
                res[k].append(s.elapsed_time(e) / ITERS)
        a, b = statistics.median(res["A"]), statistics.median(res["B"])
        print(f"{name:10s} F={F} {H}x{W}  A {a:7.4f} ms ({bpp * px / a / 1e6 / 8000:.3f})   B {b:7.4f} ms ({bpp * px / b / 1e6 / 8000:.3f})"
              f"   B/A {b / a:.3f}   rounds A {min(res['A']):.4f} .. {max(res['A']):.4f}  B {min(res['B']):.4f} .. {max(res['B']):.4f}"
              f"   outputs equal: {equal}", flush=True)


if __name__ == "__main__":
    main()
