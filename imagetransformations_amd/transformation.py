"""Drop-in for the reference's `transformation.py` per-image functions, backed by HIP.

Same names, argument meaning, return types and error behaviour as
/root/reference/transformation.py:173-354 (`apply_<x>(img: PIL.Image, ...) -> PIL.Image`)
and its driver `apply_all_transformations` (:92-170).  Each body is
    PIL image -> uint8 HWC device tensor -> libimgxf kernel(s) -> PIL image
and fails loudly when the HIP library or a ROCm device is missing (no CPU path).
Batches of frames should use `imagetransformations_amd.ops` directly and stay on the device.
"""
from __future__ import annotations

import math
import os
import random
from typing import List, Tuple

import numpy as np
import torch
from PIL import Image

from . import batched, ops, staging

# Where apply_all_transformations writes its JPEGs (the reference hard-codes a
# /Users/... path at transformation.py:13-17).  None = do not write files.
output_dir: str | None = os.environ.get("IMGXF_OUTPUT_DIR")

TRANSFORMATIONS_2D = {                      # transformation.py:95-105
    'scale': {'min': 0.9, 'max': 1.4, 'step': 0.1},
    'rotation': {'min': -22.5, 'max': 22.5, 'step': 2.5},
    'lighten_darken': {'min': -0.05, 'max': 0.05, 'step': 0.01},
    'gaussian_noise': {'min': 0.0, 'max': 0.1, 'step': 0.01},
    'translation': {'min': -50, 'max': 50, 'step': 5},
    'contrast': {'min': 0, 'max': 1, 'step': 0.1},
    'blur': {'min': 0, 'max': 5, 'step': 0.5},
    'shear': {'min': 0, 'max': 1, 'step': 0.1},
}


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("imagetransformations_amd needs a ROCm device (MI355X); none is visible "
                           "and there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _upload(img: Image.Image) -> torch.Tensor:
    """np.array(img) (HWC / HW uint8) -> device tensor."""
    arr = np.array(img)
    if arr.dtype != np.uint8:
        raise TypeError(f"only 8-bit images are supported, got mode {img.mode!r}")
    return staging.upload(arr, _device())


def _download(t: torch.Tensor) -> Image.Image:
    """Image.fromarray(device tensor): asynchronous copy into pinned memory, wait for that copy only.  An RGB frame goes
    back as RGBX and becomes a PIL image mapped onto the pinned block (staging.image_from_rgbx) while its budget lasts."""
    if t.dim() == 3 and t.shape[-1] == 3 and t.dtype == torch.uint8 and staging.zero_copy_reserve(t.shape[0] * t.shape[1] * 4):
        return staging.image_from_rgbx(staging.download(ops.permute_channels(t, (0, 1, 2, 2))).numpy())
    return Image.fromarray(staging.download(t).numpy())


def _hw(t: torch.Tensor):
    """(height, width) of a [H,W], [H,W,C] or [N,H,W,C] tensor."""
    return (t.shape[0], t.shape[1]) if t.dim() == 2 else (t.shape[-3], t.shape[-2])


def _drop_alpha(t: torch.Tensor) -> torch.Tensor:
    return ops.permute_channels(t, (0, 1, 2)) if t.dim() == 3 and t.shape[2] == 4 else t


# ------------------------------------------------------------------ scale (:173-196)
def _scale_t(t: torch.Tensor, scale_factor: float) -> torch.Tensor:
    """apply_scale on a [H,W,C] or [N,H,W,C] device tensor."""
    height, width = _hw(t)
    new_width = int(width * scale_factor)
    new_height = int(height * scale_factor)
    if scale_factor > 1.0:
        # resize + centre crop in one pass over the pixels that survive the crop
        left = (new_width - width) // 2
        top = (new_height - height) // 2
        return ops.resize_crop(t, (new_width, new_height), (left, top, left + width, top + height))
    if scale_factor < 1.0 and new_width >= 1 and new_height >= 1:
        # resize straight into its place on the black canvas (the paste at :188-194)
        canvas = ops.new(t, height, width, (0, 0, 0))
        left, top = (width - new_width) // 2, (height - new_height) // 2
        window = canvas[..., top:top + new_height, left:left + new_width, :] if t.dim() >= 3 else \
            canvas[top:top + new_height, left:left + new_width]
        ops.resize(t, (new_width, new_height), ops.RESAMPLE_LANCZOS, out=window)
        return canvas
    return ops.resize_lanczos(t, (new_width, new_height))


def apply_scale(img: Image.Image, scale_factor: float) -> Image.Image:
    return _download(_scale_t(_upload(img), scale_factor))


# ------------------------------------------------------------------ rotation (:198-201)
def _rotation_t(t: torch.Tensor, angle: float) -> torch.Tensor:
    return ops.rotate(t, -angle, ops.NEAREST, fillcolor=(0, 0, 0))


def apply_rotation(img: Image.Image, angle: float) -> Image.Image:
    return _download(_rotation_t(_upload(img), angle))


# ------------------------------------------------------------------ contrast (:203-210)
def apply_contrast(img: Image.Image, contrast_amount: float) -> Image.Image:
    t = _upload(img)
    if t.dim() == 2:
        raise IndexError("tuple index out of range")   # img_np.shape[2] on a 2-D array (:205)
    return _download(ops.scale_abs(_drop_alpha(t), contrast_amount, 0.0))


# ------------------------------------------------------------------ shear (:212-226)
def _shear_t(t: torch.Tensor, shear_factor: float) -> torch.Tensor:
    height, width = _hw(t)
    shift_in_pixels = int(math.ceil(shear_factor * height))
    matrix = (1, shear_factor, -shift_in_pixels if shear_factor > 0 else 0, 0, 1, 0)
    return ops.affine(t, matrix, (width + shift_in_pixels, height), ops.BICUBIC, fillcolor=(255, 255, 255))


def apply_shear(img: Image.Image, shear_factor: float) -> Image.Image:
    return _download(_shear_t(_upload(img), shear_factor))


# ------------------------------------------------------------------ blur (:228-257)
def _blur_ksize(blur_radius: float) -> int:
    """The reference's kernel-size rule (:239-246); 0 means "return the input object"."""
    ksize = int(blur_radius * 6)
    if ksize % 2 == 0:
        ksize += 1
    if ksize < 3 and blur_radius > 0:
        ksize = 3
    elif blur_radius == 0:
        return 0
    return ksize


# False (default): cv2.GaussianBlur by its float definition, the <= 1e-5 contract of BASELINE.json.  True (or
# IMGXF_BLUR_FIXED_POINT=1): OpenCV's uint8 fixed-point evaluation (restated, unpinned), which the reference's own output
# files sit marginally closer to (README.md)
BLUR_FIXED_POINT = os.environ.get("IMGXF_BLUR_FIXED_POINT", "0") == "1"


def apply_blur(img: Image.Image, blur_radius: float) -> Image.Image:
    """cv2.GaussianBlur by its float definition (the contract, to 1e-5 relative).  With the
    module switch BLUR_FIXED_POINT the 8-bit fixed-point evaluation of OpenCV >= 4 is used instead
    (restated and unpinned, but closer to the reference's own outputs)."""
    ksize = _blur_ksize(blur_radius)
    if ksize == 0:
        return img          # the reference hands back the input object itself (:245-246)
    t = _drop_alpha(_upload(img))
    return _download(ops.gaussian_blur(t, ksize, blur_radius, fixed_point=BLUR_FIXED_POINT))


# ------------------------------------------------------------------ brightness (:261-269)
def apply_brightness(img: Image.Image, brightness_factor: float) -> Image.Image:
    if img.mode not in ("RGB", "L"):
        raise NotImplementedError(f"apply_brightness supports RGB and L images, got {img.mode!r}")
    return _download(ops.brightness(_upload(img), 1.0 + brightness_factor))


# ------------------------------------------------------------------ gaussian noise (:272-281)
# "numpy" (default): the reference's own stream, bit-exact parity for the same np.random.seed.  Since late round 3 the
#   numbers themselves are computed on the device (numpy_stream.draw_on_device: MT19937 blocks + legacy_gauss restated, the
#   global generator's state advanced as np.random.normal would have; host draw if a sample is too close to a float32
#   rounding boundary for the device's log to be trusted).  "numpy-host" (IMGXF_NOISE_RNG=numpy-host): np.random.normal
#   on the host, as the reference itself.
# "device" (IMGXF_NOISE_RNG=device, opt-in): Philox4x32-10 + Box-Muller inside the add kernel; ONE np.random draw
# per call supplies the seed (so np.random.seed still makes a run repeatable), the pixels differ from the reference's
# for the same seed: distribution-level parity only (tests/test_gpu_noise_rng.py).  The host draw
# is ~8 of the 8.6 ms per 375 x 500 image in the batched driver.
NOISE_RNG = os.environ.get("IMGXF_NOISE_RNG", "numpy")
NOISE_DEVICE_MIN = 1 << 16                               # normals per call below which the host draws them itself


def _noise_seed() -> int:
    return int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))


def apply_gaussian_noise(img: Image.Image, noise_std: float) -> Image.Image:
    """The noise is drawn on the host from NumPy's global generator exactly as the reference
    does (same stream for the same np.random.seed), then added and clipped on the device.
    With NOISE_RNG == "device" the normals are generated on the device instead (opt-in, see above)."""
    if NOISE_RNG == "device":
        return _download(ops.add_noise_device(_upload(img), noise_std * 255, _noise_seed()))
    img_array = np.array(img)
    dev = _device()
    z = _numpy_noise([(img_array.size, noise_std * 255)], dev)[0]
    if z is None:
        z = torch.from_numpy(np.random.normal(0, noise_std * 255, img_array.shape).astype(np.float32)).to(dev)
    out = ops.add_noise(torch.from_numpy(img_array).to(dev), z.view(img_array.shape))
    return _download(out)


def _stream_device(samples: int, dev):
    """The gate of the np.random stream on the device: the device that computes a call's numbers, or None where the host draws
    them — mode "numpy-host", fewer than NOISE_DEVICE_MIN samples (normals + uniforms) in the whole call, no sample at all
    (an empty list), or no ROCm device.
    Below the gate nothing touches the device (`dev` None: the current device, looked up past it)."""
    if NOISE_RNG == "numpy-host" or samples < max(1, NOISE_DEVICE_MIN) or not torch.cuda.is_available():
        return None                                     # (a CIFAR image is 3072 normals: 50 us on the host, less than one launch)
    return _device() if dev is None else dev


def _numpy_noise(requests, dev=None, f64=False, deferred=False):
    """[(count, scale)] -> device tensors holding np.random.normal(0, scale, count) for each request (cast to float32
    unless `f64`), np.random's state advanced accordingly; [None, ...] (state untouched) when the host has to draw:
    `_stream_device`'s gate, or numpy_stream.draw_on_device refuses.
    `deferred`: the generator starts now on a side stream (numpy_stream.PendingDraw) and a function comes back that gives
    the list later — nothing else may use np.random in between; None when the gate leaves the draw to the host."""
    dev = _stream_device(sum(n for n, _ in requests), dev)
    if dev is None:
        return None if deferred else [None] * len(requests)
    from . import numpy_stream
    draw = numpy_stream.PendingDraw(requests, dev, f64).result if deferred else \
        (lambda: numpy_stream.draw_on_device(requests, dev, f64))

    def finish():
        got = draw()
        return got if got is not None else [None] * len(requests)
    return finish if deferred else finish()


def _numpy_mixed(requests, dev=None, f64=False):
    """`_numpy_noise` for np.random calls of several kinds in call order — ("normal", count, scale), ("random", count),
    ("randint", low, high); numpy_stream.draw_mixed — : device tensors for the normals (float32 unless `f64`) and the
    uniforms, Python ints for the randints, np.random's state advanced as the calls would have; None (state untouched,
    nothing on the device) when the host has to make the calls: `_stream_device`'s gate (an empty list is below it), or
    draw_mixed refuses."""
    dev = _stream_device(sum(r[1] for r in requests if r[0] != "randint"), dev)
    if dev is None:
        return None
    from . import numpy_stream
    return numpy_stream.draw_mixed(requests, dev, f64)


# ------------------------------------------------------------------ translation (:284-307)
def _translation_t(t: torch.Tensor, tx: float, ty: float) -> torch.Tensor:
    """:284-307: black canvas, crop of what stays visible, paste at max(0, int(t)) — i.e. every pixel moves by
    (int(tx), int(ty)) and what moves in from outside is black; one kernel instead of fill + copy."""
    return ops.translate(t, int(tx), int(ty), (0, 0, 0))


def apply_translation(img: Image.Image, tx: float, ty: float) -> Image.Image:
    return _download(_translation_t(_upload(img.convert('RGB') if img.mode != 'RGB' else img), tx, ty))


def apply_camera_distance(img: Image.Image, distance_factor: float) -> Image.Image:   # :309-314
    return apply_scale(img, 2.75 / distance_factor)


def apply_xy_translation_3d(img: Image.Image, tx: float, ty: float) -> Image.Image:   # :316-321
    width, height = img.size
    return apply_translation(img, int(tx * width), int(ty * height))


def apply_rotation_3d(img: Image.Image, angle: float) -> Image.Image:                 # :324-325
    return apply_rotation(img, angle)


# ------------------------------------------------------------------ background (:328-354)
def _rgb_tensor(img: Image.Image) -> torch.Tensor:
    t = _upload(img)
    if t.dim() == 2:
        raise NotImplementedError("background change expects a colour image")
    return _drop_alpha(t)


def apply_background_change(img: Image.Image, bg_color: Tuple[float, float, float]) -> Image.Image:
    bg_rgb = tuple(int(c * 255) for c in bg_color)
    rgb = _rgb_tensor(img)
    edges = ops.rgb_sobel(rgb)                            # ndimage.sobel(img.convert('L')) (:336-339), L never stored
    edge_mask = ops.percentile_mask(edges, 70)            # edges > np.percentile(edges, 70)
    foreground = ops.dilate_cross(edge_mask, 3)           # binary_dilation(iterations=3)
    return _download(ops.composite_const(rgb, bg_rgb, foreground))   # Image.composite(img, Image.new(.., bg), mask)


def apply_background_change_batch(images, bg_colors) -> List[Image.Image]:
    """`[apply_background_change(img, c) for img, c in zip(images, bg_colors)]` for PIL images of any sizes through the list
    route (`ops.background_change_list`): every image uploaded once, all of them in one block copy and two launches.
    `bg_colors`: one float triple for every image, or one per image; bytes are int(c * 255) as above.  Alpha is dropped and
    gray images are refused, as above."""
    images = list(images)
    bg_colors = list(bg_colors)
    if bg_colors and not isinstance(bg_colors[0], (tuple, list, np.ndarray)):
        bg_colors = [tuple(bg_colors)] * len(images)
    if len(bg_colors) != len(images):
        raise ValueError(f"bg_colors has {len(bg_colors)} entries for {len(images)} images")
    bg_rgb = [tuple(int(c * 255) for c in colour) for colour in bg_colors]
    for colour in bg_rgb:
        if len(colour) != 3:
            raise ValueError("a background colour is three floats (r, g, b)")
    frames = [_rgb_tensor(img) for img in images]
    return [_download(t) for t in ops.background_change_list(frames, bg_rgb)]


def apply_background_change_simple(img: Image.Image, bg_color: Tuple[float, float, float]) -> Image.Image:
    bg_rgb = tuple(int(c * 255) for c in bg_color)
    return _download(ops.blend(_rgb_tensor(img), bg_rgb, 0.3))


# ------------------------------------------------------------------ driver (:73-170)
def load_data(data_path):
    """Walk `data_path`, open every *.jpeg as RGB -> [(PIL image, path)] (:73-89)."""
    image_paths = []
    for root, _, files in os.walk(data_path):
        image_paths.extend(os.path.join(root, f) for f in files if f.lower().endswith('.jpeg'))
    images = []
    for path in image_paths:
        try:
            images.append((Image.open(path).convert("RGB"), path))
        except Exception as e:      # the reference only guards the file loading
            print(f"Failed to load image {path}: {e}")
    print(f"Loaded {len(images)} images.")
    return images


_DISPATCH = {
    'scale': apply_scale,
    'rotation': apply_rotation,
    'lighten_darken': apply_brightness,
    'gaussian_noise': apply_gaussian_noise,
    'contrast': apply_contrast,
    'shear': apply_shear,
    'blur': apply_blur,
    'translation': apply_translation,
}


def grid_values(params) -> List[float]:
    """min + j*step for j < int((max-min)/step)+1 — float artefacts included (:126-127)."""
    num_steps = int((params['max'] - params['min']) / params['step']) + 1
    return [params['min'] + j * params['step'] for j in range(num_steps)]


def plan_transformations(name: str):
    """One random draw per transform type in the reference's order -> [(type, args, filename)].
    Consumes `random` exactly like the loop at transformation.py:119-139."""
    plan = []
    for transform_type, params in TRANSFORMATIONS_2D.items():
        values = grid_values(params)
        if transform_type == 'translation':
            tx = random.choice(values)
            ty = random.choice(values)
            plan.append((transform_type, (tx, ty), f"{name}_{transform_type}_{tx}_{ty}_corrupted.jpg"))
        else:
            value = random.choice(values)
            plan.append((transform_type, (value,), f"{name}_{transform_type}_{value}_corrupted.jpg"))
    return plan


JPEG_ON_DEVICE = os.environ.get("IMGXF_JPEG_DEVICE", "0") == "1"


JPEG_DEVICE_PARAMS = ("quality", "subsampling", "optimize", "progressive", "progression")   # what the device writer takes


def _device_jpeg_values(params) -> bool:
    """Values the device writer takes as Pillow does: quality an int 1..100, subsampling one of jpeg.SUBSAMPLING.  Pillow
    also accepts others (quality -1 or a preset name, subsampling 3, "4:1:1" or a bool), which stay with it."""
    from . import jpeg
    q, s = params.get("quality", 75), params.get("subsampling", -1)
    return (isinstance(q, int) and not isinstance(q, bool) and 1 <= q <= 100
            and isinstance(s, (int, str)) and not isinstance(s, bool) and s in jpeg.SUBSAMPLING
            and all(isinstance(params.get(k, False), bool) for k in ("progressive", "progression")))


def save_image(img: Image.Image, path: str, **params) -> None:
    """The reference's `transformed.save(path)` (:161-162), and `img.save(path, **params)`.  With `JPEG_ON_DEVICE` (or
    IMGXF_JPEG_DEVICE=1) an RGB or "L" image bound for a *.jpg / *.jpeg file, with no parameters beyond quality (1..100) /
    subsampling (jpeg.SUBSAMPLING) / optimize / progressive or progression (bools), is encoded by the GPU writer (`jpeg.encode`: the file Pillow would write, byte for byte);
    every other mode / format / parameter, and images carrying a comment Pillow would embed, go through Pillow.  Without
    parameters only RGB images take the device, as before."""
    device = (JPEG_ON_DEVICE and path.lower().endswith((".jpg", ".jpeg")) and "comment" not in img.info and min(img.size) > 0
              and set(params) <= set(JPEG_DEVICE_PARAMS) and (img.mode == "RGB" or (img.mode == "L" and params))
              and _device_jpeg_values(params))
    if device:
        from . import jpeg
        frame = _upload(img)
        frame = frame[..., None] if frame.dim() == 2 else frame      # "L": [H, W, 1], whatever its width
        kw = {k: v for k, v in params.items() if k not in ("progressive", "progression")}
        if params.get("progressive", False) or params.get("progression", False):   # Pillow: either name
            kw["progressive"] = True
        data = jpeg.encode(frame[None], **kw)[0]
        with open(path, "wb") as f:
            f.write(data)
    else:
        img.save(path, **params)


def apply_jpeg_compression(image: Image.Image, quality: int = 75) -> Image.Image:
    """An addition the reference does not have: `image` as it reads back after `image.save(path, "JPEG", quality=quality)`
    and `Image.open(path)` — the JPEG-compression corruption of the ImageNet-C family, and what every file the reference's
    driver saves does to its frame — computed on the device without a file (`jpeg.roundtrip`).  RGB and "L" images; the
    result has the input's mode and size and Pillow's pixels, bit for bit."""
    if image.mode not in ("RGB", "L"):
        raise ValueError(f"apply_jpeg_compression takes RGB and 'L' images, not mode {image.mode!r}")
    from . import jpeg
    frame = _upload(image)
    if image.mode == "L":                              # [1, H, W, 1]: a [1, H, 3] tensor would read as one RGB frame
        return _download(jpeg.roundtrip(frame[None, :, :, None], quality)[0, :, :, 0])
    return _download(jpeg.roundtrip(frame[None], quality)[0])


# The batched driver on frames of different sizes (driver_list.apply_list: seven of the eight types of all sizes in at most
# two record-driven device passes per chunk, instead of one launch per (size, type, drawn value)).  "auto": a chunk that
# holds more than one frame size takes it, a uniform chunk keeps the grouped route; "0": never; "1": always.  The twelve-type
# driver (transformations_code.apply_all_transformations_batched) reads the same knob: eleven types in one pass per call.
DRIVER_LIST = os.environ.get("IMGXF_DRIVER_LIST", "auto")
DRIVER = os.environ.get("IMGXF_DRIVER", "batched")       # "per-image": apply_all_transformations runs the reference's literal loop
DRIVER_CHUNK = 256                                        # images per pass of the batched driver inside apply_all_transformations


def apply_all_transformations(images):
    """images: [(PIL image, path)] -> list of transformed PIL images (8 per input), /root/reference/transformation.py:92-170.
    Same draws (`random`, `np.random`), same names, same order, same pixels as the literal loop
    (`apply_all_transformations_per_image`, which tests/test_gpu_facade.py holds it against); since late round 3 the work is
    done DRIVER_CHUNK images at a time by the batched driver — images of one size share their uploads, launches and copies
    back.  A chunk that holds more than one image size (`DRIVER_LIST`, "auto") runs everything but blur in at most two
    `driver_list.apply_list` calls, whatever the number of sizes: the same draws, names, order and pixels.  A chunk with an
    image that is not 8-bit RGB, and `IMGXF_DRIVER=per-image`, take the literal loop."""
    if DRIVER == "per-image":
        return apply_all_transformations_per_image(images)
    images = list(images)
    transformed_images = []
    for c0 in range(0, len(images), DRIVER_CHUNK):
        chunk = images[c0:c0 + DRIVER_CHUNK]
        if all(batched.is_rgb(img) for img, _ in chunk):
            transformed_images.extend(apply_all_transformations_batched(chunk))
        else:
            transformed_images.extend(apply_all_transformations_per_image(chunk, _progress=False))
        done = c0 + len(chunk)
        for mark in range((c0 // 1000 + 1) * 1000, done + 1, 1000):     # the reference's progress line, per thousand images
            print(f"Processed {mark}/{len(images)} original images, created {8 * mark} transformed images")
    return transformed_images


def apply_all_transformations_per_image(images, _progress: bool = True):
    """The reference's loop, call by call: one upload, one launch and one copy back per transformation."""
    transformed_images = []
    total_transforms = 0
    for i, (img, path) in enumerate(images):
        name = os.path.splitext(os.path.basename(path))[0]
        for transform_type, args, new_filename in plan_transformations(name):
            transformed_img = _DISPATCH[transform_type](img, *args)
            if output_dir is not None:
                save_image(transformed_img, os.path.join(output_dir, new_filename))
            transformed_images.append(transformed_img)
            total_transforms += 1
        if _progress and (i + 1) % 1000 == 0:
            print(f"Processed {i + 1}/{len(images)} original images, created {total_transforms} transformed images")
    return transformed_images


def apply_all_transformations_batched(images):
    """`apply_all_transformations_batched_named` + the reference's save step (:159-162).  With `output_dir` set the files are
    written by the device writer (byte-identical to Pillow's `save`, tests/test_gpu_jpeg.py) while the images still come back;
    `IMGXF_SAVE=pillow` keeps Pillow's encoder."""
    if output_dir is not None and os.environ.get("IMGXF_SAVE", "device") == "device":
        return [img for _, img in _batched_to_files(images, output_dir, tee=True)]
    transformed_images = []
    for new_filename, img in apply_all_transformations_batched_named(images):
        if output_dir is not None:
            save_image(img, os.path.join(output_dir, new_filename))
        transformed_images.append(img)
    return transformed_images


def apply_all_transformations_batched_to_files(images, out_dir: str) -> List[str]:
    """The batched driver with the save step on the device and NO images copied back: returns the file names in output order
    (`_batched_to_files`)."""
    return [name for name, _ in _batched_to_files(images, out_dir, tee=False)]


def _batched_to_files(images, out_dir: str, tee: bool):
    """The batched driver with the save step (:159-162) on the device too: every group's result goes from the transform
    kernels straight into the JPEG writer (`jpeg.encode`), and only the files — a tenth of a byte per pixel for
    photographs instead of three — cross PCIe.  Same draws, names, order and FILES as `apply_all_transformations_batched`
    with `output_dir` set (Pillow's encoder): tests/test_gpu_jpeg.py.  Returns [(file name, image or None)] in output order:
    `tee` also copies the results back as PIL images (apply_all_transformations_batched with `output_dir` set)."""
    os.makedirs(out_dir, exist_ok=True)
    # Groups are small (a handful of frames per transformation type and parameter) and a writer call costs ~0.4 ms of host
    # time whatever its size: the results of ALL shapes are held together, as the groups' own output tensors, and encoded
    # SINK_FRAMES at a time by the list writer (`jpeg.encode_list_views`: one call, a fixed number of launches, whatever
    # the mix of sizes).  A flush that holds a single shape keeps the batch writer (_encode_held).
    held: list = [[], [], 0, 0]                           # [group outputs], [names], frames, bytes
    written: set = set()                                  # names the sink has put on disk

    def flush() -> None:
        # (the files are written here, by this thread: a side thread pays a GIL hand-over per system call while this one
        # computes — 110 us per file against 19 us — and several threads queue on the directory's lock, 213 us per file)
        outs, names = held[0], held[1]
        held[:] = [[], [], 0, 0]
        if not outs:
            return
        for name, data in zip(names, _encode_held(outs)):
            with open(os.path.join(out_dir, name), "wb") as f:
                f.write(data)
        written.update(names)

    def sink(out: torch.Tensor, names: List[str]) -> None:
        on_device = [n.lower().endswith((".jpg", ".jpeg")) for n in names]
        if all(on_device) and out.dim() == 4 and out.shape[-1] == 3:
            held[0].append(out); held[1].extend(names); held[2] += out.shape[0]; held[3] += out.numel()
            if held[2] >= SINK_FRAMES or held[3] >= SINK_BYTES:
                flush()
        else:                                             # another format: Pillow writes it
            host = staging.download(out).numpy()
            for j, name in enumerate(names):
                Image.fromarray(host[j]).save(os.path.join(out_dir, name))
            written.update(names)

    named = apply_all_transformations_batched_named(images, _sink=sink, _tee=tee)
    sunk = set()
    if tee:                                               # the names the sink has written: everything else is saved below
        sunk = set(held[1]) | written
    for name, img in named:
        if isinstance(img, torch.Tensor):                 # apply_blur's radius-0 pass-through of a device frame
            sink(img[None], [name])
        elif img is not None and name not in sunk:        # per-image path (not RGB) or apply_blur's radius-0 pass-through
            save_image(img, os.path.join(out_dir, name))
    flush()
    return named


SINK_FRAMES = 1024                                        # frames per writer call in the device-save drivers ...
SINK_BYTES = 2 << 30                                      # ... or this many bytes of them (4K frames: 86 per call), whichever comes first


def _encode_held(outs: List[torch.Tensor]):
    """The files (memoryviews, in order) of the frames of `outs`, [B_i, H_i, W_i, 3] device tensors.  Mixed shapes: every
    frame goes, as a view of its group's output, through ONE `jpeg.encode_list_views` call.  A single shape: the batch
    writer `jpeg.encode_views` on the (concatenated) batch, the faster route on a uniform batch (1024 frames of 375 x 500:
    4.85 ms against the list route's 5.88 ms, profiles/jpeg_encode_list.txt)."""
    from . import jpeg
    if len({tuple(o.shape[1:]) for o in outs}) == 1:
        return jpeg.encode_views(outs[0] if len(outs) == 1 else torch.cat(outs))
    return jpeg.encode_list_views([o[j] for o in outs for j in range(o.shape[0])])


_TENSOR_FNS = {                                           # type -> the apply_<type> body on a [B, H, W, 3] device batch
    'scale': _scale_t,
    'rotation': _rotation_t,
    'lighten_darken': lambda t, b: ops.brightness(t, 1.0 + b),
    'contrast': lambda t, a: ops.scale_abs(t, a, 0.0),
    'shear': _shear_t,
    'translation': _translation_t,
}


def _blur_group(batch: torch.Tensor, blur_radius: float):
    """apply_blur on a batch; None for radius 0, where the reference hands back the input object itself (:245-246)."""
    ksize = _blur_ksize(blur_radius)
    return ops.gaussian_blur(batch, ksize, blur_radius, fixed_point=BLUR_FIXED_POINT) if ksize else None


def apply_all_transformations_batched_named(images, _sink=None, _tee=False):
    """`apply_all_transformations` with the work grouped for the GPU, returning
    [(file name, image)] in the reference's output order and saving nothing: same draws (`random` per
    transform type per image, `np.random` for the noise, in the reference's order), same file
    names, same outputs in the same order — but every image is uploaded once, and all images
    of one size that drew the same (type, value) go through ONE batched launch.  Images that
    are not 8-bit RGB take the per-image path.  images: [(PIL image, path)] — or [(frame, path)] with [H, W, 3] uint8
    DEVICE tensors as the device JPEG reader returns them (`jpeg_decode.decode`): those are never copied to the host.  `_sink(out, names)`, when given,
    consumes a group's result ON THE DEVICE ([B, H, W, 3] tensor + its file names) instead of it being copied back:
    those entries come back as (file name, None).  With `DRIVER_LIST` ("auto": more than one image size among `images`)
    the eight types of ALL sizes run in at most two `driver_list.apply_list` calls instead of one launch per
    (size, type, value) — the second one for the noise entries, once their numbers have been collected; entries that call
    refuses (among them the float blurs that the per-type dispatcher serves with another kernel family than the list's:
    16-byte rows, by and large), radius-0 blurs and the Philox noise keep the groups."""
    if DRIVER_LIST not in ("auto", "0", "1"):
        raise ValueError(f'DRIVER_LIST / IMGXF_DRIVER_LIST must be "auto", "0" or "1", got {DRIVER_LIST!r}')
    dev = _device()
    plans, noise = [], {}
    draws = []                                          # (i, k, (h, w, 3), scale): np.random.normal calls in the per-image loop's order
    for i, (img, path) in enumerate(images):
        name = os.path.splitext(os.path.basename(path))[0]
        plan = plan_transformations(name)
        plans.append(plan)
        for k, (transform_type, args, _) in enumerate(plan):
            if transform_type == 'gaussian_noise':      # same np.random stream as the per-image loop
                w, h = batched.size_of(img)
                if NOISE_RNG == "device":               # opt-in: one seed per image instead of h * w * 3 normals
                    noise[(i, k)] = _noise_seed()
                else:
                    draws.append((i, k, (h, w, 3), args[0] * 255))
    noise_later = None
    if draws:
        # nothing else touches np.random between these calls (the grid values come from `random`): one pass over the stream
        # on the device serves them all, or the host makes them one by one.  The MT19937 block kernel (one workgroup) starts
        # NOW on a side stream; the numbers are collected when the first noise group comes up, after the other transformation
        # types have been queued (the noise groups of a size run last).
        noise_later = _numpy_noise([(h * w * c, scale) for _, _, (h, w, c), scale in draws], dev, deferred=True)
        if noise_later is None:
            for (i, k, shape, scale) in draws:
                noise[(i, k)] = np.random.normal(0, scale, shape).astype(np.float32)

    def collect_noise():
        nonlocal noise_later
        if noise_later is None:
            return
        got, noise_later = noise_later(), None
        for z, (i, k, shape, scale) in zip(got, draws):
            noise[(i, k)] = z.view(shape) if z is not None else np.random.normal(0, scale, shape).astype(np.float32)

    def per_image(i):                                   # not 8-bit RGB, rare: keep the reference's behaviour exactly
        out = []
        for transform_type, args, _ in plans[i]:
            if transform_type == 'gaussian_noise':
                raise NotImplementedError("batched driver expects RGB images (load_data converts them)")
            out.append(_DISPATCH[transform_type](images[i][0], *args))
        return out

    def run_group(transform_type, args, batch, entries):
        if transform_type == 'blur':
            return _blur_group(batch, args[0])
        if transform_type == 'gaussian_noise' and NOISE_RNG == "device":
            out = torch.empty_like(batch)               # every image has its own seed (as the per-image call draws it)
            for j, (_, i, k) in enumerate(entries):
                out[j] = ops.add_noise_device(batch[j], args[0] * 255, noise[(i, k)])
            return out
        if transform_type == 'gaussian_noise':
            collect_noise()
            zs = [noise[(i, k)] for _, i, k in entries]
            return ops.add_noise(batch, torch.stack(zs) if isinstance(zs[0], torch.Tensor) else staging.upload(zs, dev))
        return _TENSOR_FNS[transform_type](batch, *args)

    # Frames of different sizes (DRIVER_LIST): everything but the radius-0 blur (the input object itself) and the opt-in
    # Philox noise leaves the groups and runs in two list calls for the whole chunk, the noise entries in the second one,
    # after the other work has been queued.
    def list_phase(transform_type, args):
        if transform_type == 'blur':
            return 0 if _blur_ksize(args[0]) != 0 else None
        if transform_type == 'gaussian_noise' and NOISE_RNG == "device":
            return None
        return 1 if transform_type == 'gaussian_noise' else 0

    def run_list(phase, frames, items):
        from . import driver_list
        if phase == 1:
            collect_noise()
        entries = []
        for f, transform_type, args, i, k in items:
            if transform_type == 'gaussian_noise':
                z = noise[(i, k)]
                args = (z if isinstance(z, torch.Tensor) else staging.upload(z, dev),)
            entries.append((f, transform_type, args))
        return driver_list.apply_list_block(frames, entries)

    sizes = {batched.size_of(img) for img, _ in images if batched.is_rgb(img)}
    use_list = DRIVER_LIST == "1" or (DRIVER_LIST == "auto" and len(sizes) > 1)
    # (noise groups last: their numbers come from the side stream's generator, which runs meanwhile)
    results = batched.run_grouped([img for img, _ in images], plans, dev, run_group, order=lambda g: g[0] == 'gaussian_noise',
                                  other=per_image, sink=_sink, tee=_tee, list_route=(list_phase, run_list) if use_list else None)
    return [(new_filename, results[i][k]) for i, plan in enumerate(plans) for k, (_, _, new_filename) in enumerate(plan)]
