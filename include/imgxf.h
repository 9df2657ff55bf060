/*
 * imgxf.h — C-ABI of libimgxf.so: MI355X (gfx950) HIP kernels for the per-pixel
 * transform hot path of aaryaamoharir/ImageTransformations.
 *
 * The reference has no FFI of its own: its boundary is a set of Python functions
 * (`apply_<x>(img: PIL.Image, params) -> PIL.Image`, /root/reference/transformation.py:173-354,
 * and `TransformationPool.<x>`, /root/reference/pipenline/cifar_image_transformations.py:37-129)
 * whose bodies call Pillow / OpenCV / SciPy / NumPy C kernels.  Each entry point below
 * replaces ONE of those third-party calls; the call site it replaces is cited.  The
 * Python facade (imagetransformations_amd/transformation.py) binds these with ctypes
 * exactly as INTEGRATION.md shows.
 *
 * Conventions
 *   - every function returns IMGXF_OK (0), a negative imgxf error, or a positive hipError_t;
 *     nothing throws; nothing allocates or synchronises unless its comment says so;
 *   - all pixel pointers are DEVICE pointers (e.g. torch tensor .data_ptr()); the caller owns
 *     every buffer; `stream` is a hipStream_t (NULL = the default stream); calls are ordered
 *     by the stream only and are re-entrant;
 *   - images are interleaved (HWC) batches described by imgxf_view; strides are in BYTES;
 *     src and dst must not overlap unless the comment says in-place is allowed;
 *   - small host-side parameter arrays (kernels, matrices, colours) are HOST pointers that
 *     are copied into the kernel arguments before the call returns.
 */
#ifndef IMGXF_H
#define IMGXF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMGXF_VERSION 100 /* 0.1.0 */

enum {
    IMGXF_OK = 0,
    IMGXF_ERR_NULL = -1,        /* a required pointer is NULL */
    IMGXF_ERR_SHAPE = -2,       /* n/h/w/c or strides inconsistent between views */
    IMGXF_ERR_ARG = -3,         /* scalar argument out of range */
    IMGXF_ERR_UNSUPPORTED = -4, /* valid request this build has no kernel for */
    IMGXF_ERR_WORKSPACE = -5,   /* workspace too small */
    IMGXF_ERR_NO_DEVICE = -6    /* no gfx950-compatible device / code object */
};

/* A batch of n interleaved frames: pixel (f,y,x,ch) lives at
 * data + f*frame_stride + y*row_stride + (x*c + ch)*elem_size. */
typedef struct imgxf_view {
    void*   data;
    int32_t n, h, w, c;
    int64_t row_stride;
    int64_t frame_stride;
} imgxf_view;

enum { IMGXF_BORDER_REFLECT_101 = 0, /* gfedcb|abcdefgh|gfedcba (OpenCV default) */
       IMGXF_BORDER_REFLECT = 1      /* dcba|abcd|dcba (SciPy ndimage 'reflect') */ };

enum { IMGXF_FILTER_NEAREST = 0, IMGXF_FILTER_BILINEAR = 1, IMGXF_FILTER_BICUBIC = 2 };

enum { IMGXF_SOBEL_X_WRAP = 0,    /* scipy.ndimage.sobel(u8, axis=-1): result mod 256 */
       IMGXF_SOBEL_Y_WRAP = 1,    /* axis=0 */
       IMGXF_SOBEL_MAGNITUDE = 2  /* sat_u8(rint(sqrt(Gx^2+Gy^2))) — benchmark configs[2] */ };

int         imgxf_version(void);
const char* imgxf_strerror(int code);
/* Number of visible HIP devices whose architecture this library was built for (>=0),
 * or a negative error.  Does not create a context on any device. */
int         imgxf_device_count(void);
/* The IMGXF_* tuning / routing environment variables are read once, at the first call that needs
 * one.  This re-reads them (not thread-safe against concurrent launches; for tests and A/B tools
 * that change a knob inside one process).  No reference counterpart (build infrastructure). */
int         imgxf_reload_knobs(void);
/* Measurement aid for bench.py (no reference counterpart): one wave spins for `ticks_100mhz` ticks
 * of the constant 100 MHz counter and writes {delta s_memtime, delta s_memrealtime} to the two
 * uint64 at `out2_u64` (device memory); shader clock in MHz = 100 * out[0] / out[1].  Launch it on
 * a side stream while the kernels of interest run to see the clock they are granted. */
int         imgxf_probe_sclk(void* out2_u64, unsigned int ticks_100mhz, void* stream);

/* ---- a1: cv2.GaussianBlur(img,(k,k),sigma)  transformation.py:249 -------------------
 * Separable Gaussian, BORDER_REFLECT_101, fp32 accumulate, round-half-even, saturate.
 * c in {1,3,4}; ksize odd, 1..31.  sigma<=0 as OpenCV: the binomial table for ksize <= 7,
 * sigma = 0.3*((k-1)*0.5-1)+0.8 beyond.
 * `dst_f32` (optional, may be NULL): if given, a float view of the same n,h,w,c that
 * receives the pre-quantisation fp32 values (diagnostic; used by the parity tests). */
int imgxf_gaussian_u8(const imgxf_view* src, const imgxf_view* dst, int ksize, double sigma,
                      const imgxf_view* dst_f32, void* stream);

/* Generic separable correlation with host-given fp32 taps (kx along x, ky along y). */
int imgxf_sepconv_u8(const imgxf_view* src, const imgxf_view* dst, const float* kx, int nkx,
                     const float* ky, int nky, int border, const imgxf_view* dst_f32,
                     void* stream);

/* The same filter the way OpenCV >= 4 most likely evaluates it for 8-bit images (its fixed-point
 * path; restated, cv2 is not installed — PARITY UNPINNED): taps quantised to 8 fractional bits
 * (getGaussianKernelFixedPoint_ED: error-diffused rounding, centre = 256 - rest), 8.8 rows,
 * 16.16 columns, (v + 2^15) >> 16.  Not the contract path (that is the float definition above);
 * offered because the reference's own JPEG outputs sit closer to it.
 * sepconv_fixed: host-given 8.8 integer taps, each axis summing to <= 256. */
int imgxf_gaussian_cv_fixed_u8(const imgxf_view* src, const imgxf_view* dst, int ksize,
                               double sigma, void* stream);
int imgxf_sepconv_fixed_u8(const imgxf_view* src, const imgxf_view* dst, const uint16_t* kx,
                           int nkx, const uint16_t* ky, int nky, int border, void* stream);

/* ---- a5: cv2.filter2D(img,-1,kernel)  cifar_image_transformations.py:118 ------------
 * Dense kh x kw correlation, centre anchor, fp32 accumulate, round-half-even, saturate.
 * kernel: HOST pointer, row-major kh*kw floats; kh,kw odd, <= 15. */
int imgxf_conv2d_u8(const imgxf_view* src, const imgxf_view* dst, const float* kernel, int kh,
                    int kw, int border, void* stream);
/* HOST only, no device needed: whether imgxf_conv2d_u8 hands this kernel to the separable kernels
 * (*separable = 1; images of 1, 3 or 4 channels, IMGXF_CONV2D_NO_SEPARABLE unset) and, if so, the
 * taps it hands on: kx[kw] = the row of the entry of largest magnitude P, ky[kh] = its column / P.
 * Accepted when every tap has |K[j][i] - ky[j] kx[i]| <= 1e-6 |K[j][i]| in double; kx, ky are left
 * untouched otherwise.  Same kh, kw limits as imgxf_conv2d_u8. */
int imgxf_conv2d_separable_host(const float* kernel, int kh, int kw, int* separable, float* kx,
                                float* ky);

/* ---- a4: scipy.ndimage.sobel(gray_u8)  transformation.py:339 ------------------------
 * src, dst: c == 1.  variant: IMGXF_SOBEL_*.  Border: SciPy 'reflect'. */
int imgxf_sobel_u8(const imgxf_view* src, const imgxf_view* dst, int variant, void* stream);
/* Fused benchmark configs[2]: RGB(c==3) -> L (Pillow weights) -> Gx,Gy -> magnitude -> u8 (c==1). */
int imgxf_rgb_sobel_mag_u8(const imgxf_view* src, const imgxf_view* dst, void* stream);
/* Same fusion for every variant of imgxf_sobel_u8: RGB in, Pillow L on the fly, one u8 plane out
 * (apply_background_change's edge image without materialising L, transformation.py:336-339). */
int imgxf_rgb_sobel_u8(const imgxf_view* src, const imgxf_view* dst, int variant, void* stream);
/* HOST only, no device needed: what imgxf_sobel_u8 (src c == 1) or imgxf_rgb_sobel_u8 (src c == 3) launches
 * for these views — addresses, strides and IMGXF_NO_MARCH read as the entry points read them, the same view
 * checks and error codes.  A batch above 65535 frames runs in several launches; the record is the first one's.
 * out[IMGXF_SOBEL_PLAN_INTS] (all 0 for an empty view):
 *   [0] 1 = marching kernel, 0 = tiled kernel        [1] 1024-pixel strips per row     (marching only)
 *   [2] strips per workgroup (marching only)          [3] rows per wave and chunk       (marching only)
 *   [4] row chunks (marching only)                    [5] row chunks before the split that fills the chip (marching only)
 *   [6] [7] [8] grid x, y, z                          [9] threads per workgroup
 *   [10] dynamic LDS bytes                            [11] launches */
enum { IMGXF_SOBEL_PLAN_INTS = 12 };
int imgxf_sobel_plan_host(const imgxf_view* src, const imgxf_view* dst, int* out);

/* ---- a2/a2'/shear: Image.transform(size, AFFINE, m, resample, fillcolor) -------------
 * transformation.py:200 (rotate -> NEAREST), :217-224 (shear -> BICUBIC); BILINEAR is
 * benchmark configs[3].  m[6]: HOST pointer, destination->source matrix exactly as Pillow
 * takes it.  dst gives the output size.  fill[4]: HOST pointer (per channel), NULL = zeros.
 * NEAREST reproduces libImaging affine_fixed (16.16) bit-exactly when m[1]!=0 or m[3]!=0;
 * pure scale/translate NEAREST matrices need imgxf_affine_scale_nearest_u8.  Where libImaging
 * itself leaves affine_fixed — check_fixed fails at a corner of the output, |x m0 + y m1 + m2|
 * or |x m3 + y m4 + m5| >= 32768 at (0,0), (w,0), (0,h), (w,h), and its double loop runs — or a
 * coefficient of the 16.16 matrix fits no int, NEAREST returns IMGXF_ERR_UNSUPPORTED and
 * launches nothing (the rule of imgxf_affine_list_u8).
 * precise != 0: coordinates and interpolation in fp64 (bit-exact with Pillow);
 * precise == 0: fp64 coordinates, fp32 interpolation (<=1e-5 relative before truncation).
 * `dst_f32` (optional, may be NULL; BILINEAR/BICUBIC only): float view of dst's n,h,w,c that
 * receives the pre-truncation interpolated values (diagnostic; used by the parity tests). */
int imgxf_affine_u8(const imgxf_view* src, const imgxf_view* dst, const double* m, int filter,
                    const uint8_t* fill, int precise, const imgxf_view* dst_f32, void* stream);
/* libImaging ImagingScaleAffine (NEAREST with m[1]==m[3]==0): source indices are walked on
 * one device lane per axis by the same repeated double additions Pillow performs, into
 * `workspace` (device, 4-byte aligned, >= 4*(dst->w + dst->h + 2) bytes). */
int imgxf_affine_scale_nearest_u8(const imgxf_view* src, const imgxf_view* dst, const double* m,
                                  const uint8_t* fill, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* ---- a3: img.resize((nw,nh), LANCZOS)  transformation.py:179 -------------------------
 * Two-pass integer resample (22-bit coefficients computed on the host in double exactly as
 * libImaging precompute_coeffs/normalize_coeffs_8bpc).  A plan owns the device coefficient
 * tables and the uint8 intermediate for up to `max_frames` frames; create/destroy allocate,
 * synchronise and must not be called inside stream capture; the resize call only launches.
 * A plan may be in use on one stream at a time (its intermediate is shared). */
typedef struct imgxf_lanczos_plan imgxf_lanczos_plan;
int imgxf_lanczos_plan_create(imgxf_lanczos_plan** plan, int in_h, int in_w, int out_h,
                              int out_w, int c, int max_frames);
int imgxf_lanczos_plan_destroy(imgxf_lanczos_plan* plan);
int imgxf_resize_lanczos_u8(const imgxf_lanczos_plan* plan, const imgxf_view* src,
                            const imgxf_view* dst, void* stream);
/* The same machinery with Resample.c's other filters — Image.resize's default BICUBIC is what
 * rand_crop uses (fall_2025/transformations_code:43-48).  `filter` takes Pillow's Resampling
 * values; the plan is run and destroyed with the two calls above. */
enum { IMGXF_RESAMPLE_LANCZOS = 1, IMGXF_RESAMPLE_BILINEAR = 2, IMGXF_RESAMPLE_BICUBIC = 3,
       IMGXF_RESAMPLE_BOX = 4, IMGXF_RESAMPLE_HAMMING = 5 };
int imgxf_resample_plan_create(imgxf_lanczos_plan** plan, int in_h, int in_w, int out_h,
                               int out_w, int c, int max_frames, int filter);
/* Resize + crop in one: the plan produces only rows [wy, wy+wh) x columns [wx, wx+ww) of the
 * out_h x out_w result (dst of the resize call is wh x ww) and filters only the source rows and
 * output columns that window needs — apply_scale's centre crop (transformation.py:182-187)
 * without computing the pixels it throws away.  Needs out_w != in_w and out_h != in_h. */
int imgxf_resample_plan_create_window(imgxf_lanczos_plan** plan, int in_h, int in_w, int out_h,
                                      int out_w, int c, int max_frames, int filter,
                                      int wx, int wy, int ww, int wh);
/* Stream-safe form: with max_frames == 0 a plan holds only its immutable coefficient tables; the
 * uint8 H -> V intermediate ([n][rows the window's taps touch][out_w][c] bytes, 0 for single-pass
 * plans) is a caller-provided, stream-ordered workspace, so one plan may run on any number of
 * streams and batch sizes at once and the call neither allocates nor frees (graph-capture safe).
 * Replaces the shared-intermediate contract of imgxf_resize_lanczos_u8 above. */
int imgxf_resample_workspace_bytes(const imgxf_lanczos_plan* plan, int n, size_t* bytes);
int imgxf_resample_ws_u8(const imgxf_lanczos_plan* plan, const imgxf_view* src, const imgxf_view* dst,
                         void* workspace, size_t workspace_bytes, void* stream);
/* The workspace THIS call needs: 0 when the two views let the fused kernel run (see
 * imgxf_resample_plan_kernel), else imgxf_resample_workspace_bytes(plan, src->n). */
int imgxf_resample_workspace_bytes_for(const imgxf_lanczos_plan* plan, const imgxf_view* src,
                                       const imgxf_view* dst, size_t* bytes);
/* Which kernels a two-pass plan runs on 4-byte aligned views: *ksteps = 0 -> the H and V vector
 * kernels through the intermediate; 1..3 -> both passes fused on the i8 matrix cores
 * (csrc/resample_mfma.inc, no intermediate traffic), the value being the 32-byte k-steps of its
 * horizontal product.  Same bytes either way; IMGXF_RESAMPLE_NO_MFMA=1 forces the former. */
int imgxf_resample_plan_kernel(const imgxf_lanczos_plan* plan, int* ksteps);
/* Which kernels a call with THESE views runs (alignment and strides decide with the plan; the views need no valid
 * memory behind them), with the knobs now in force and a 16-byte aligned workspace:
 *   route[0]  k-steps of the fused matrix-core kernel when it runs (then the other four are 0), else 0
 *   route[1]  IMGXF_ROUTE_H_*: the horizontal kernel (NONE: out_w == in_w, the pass is skipped)
 *   route[2]  its window KP (8, 12, 16) for FAST and LDS, the channel count it is instantiated for when GENERIC
 *   route[3]  IMGXF_ROUTE_V_*: the vertical kernel (NONE: out_h == in_h)
 *   route[4]  FAST: its window KP (= the plan's coefficients per row); V4: the union window KU (12); GENERIC: 0
 * The launch asks the same function, so the answer is what runs. */
enum { IMGXF_ROUTE_H_NONE = 0, IMGXF_ROUTE_H_GENERIC = 1, IMGXF_ROUTE_H_FAST = 2, IMGXF_ROUTE_H_LDS = 3 };
enum { IMGXF_ROUTE_V_NONE = 0, IMGXF_ROUTE_V_GENERIC = 1, IMGXF_ROUTE_V_FAST = 2, IMGXF_ROUTE_V_V4 = 3 };
int imgxf_resample_plan_route(const imgxf_lanczos_plan* plan, const imgxf_view* src, const imgxf_view* dst,
                              int route[5]);

/* ---- a6: elementwise colour maps ------------------------------------------------------*/
/* Pillow convert('L') transformation.py:336: (19595R+38470G+7471B+0x8000)>>16. src c in {3,4}, dst c==1 */
int imgxf_rgb2l_u8(const imgxf_view* src, const imgxf_view* dst, void* stream);
/* cv2.convertScaleAbs(img, alpha, beta) transformation.py:207: sat_u8(rint(|alpha*p+beta|)). In-place ok. */
int imgxf_scale_abs_u8(const imgxf_view* src, const imgxf_view* dst, float alpha, float beta,
                       void* stream);
/* Image.blend(im1, im2, alpha) (libImaging Blend.c) transformation.py:267,354:
 * f32 `p1 + alpha*(p2-p1)`; 0<=alpha<=1 truncates, else clip then truncate.
 * im2 == NULL: the second image is the solid colour `color2[c]` (HOST pointer).
 * im1 == NULL: the first image is the solid colour `color1[c]`.  In-place ok. */
int imgxf_blend_u8(const imgxf_view* im1, const uint8_t* color1, const imgxf_view* im2,
                   const uint8_t* color2, const imgxf_view* dst, float alpha, void* stream);
/* transformation.py:275-278: clip(f32(p)+noise,0,255) truncated; noise: float view, same n,h,w,c. */
int imgxf_add_noise_u8(const imgxf_view* src, const imgxf_view* noise_f32, const imgxf_view* dst,
                       void* stream);
/* The same step with the noise tensor GENERATED ON THE DEVICE (opt-in, IMGXF_NOISE_RNG=device in the facade): the host's
 * np.random.normal(0, sigma, shape).astype(f32) at transformation.py:274 is replaced by Philox4x32-10 (key = seed,
 * counter = offset / 4 + element index / 4) + Box-Muller in fp32, scaled by `sigma` (= noise_std * 255); then
 * clip(f32(p) + noise, 0, 255) truncated as above.  A different random stream than NumPy's MT19937: distribution-level
 * parity only.  `offset` (a multiple of 4) numbers the first normal of this call, so frames of one
 * logical batch can be processed in several calls with identical results.  In-place ok. */
int imgxf_add_noise_philox_u8(const imgxf_view* src, const imgxf_view* dst, float sigma, uint64_t seed,
                              uint64_t offset, void* stream);
/* The raw uint32 stream behind it (tests: Random123 known-answer vectors): count (multiple of 4) values to dst_u32. */
int imgxf_philox4x32_u32(void* dst_u32, int64_t count, uint64_t seed, uint64_t offset, void* stream);
/* cv2.cvtColor channel permutations (RGB2BGR, RGBA2RGB, ...) transformation.py:206,233-235,252:
 * dst[..., j] = src[..., perm[j]] for j < dst->c.  perm: HOST pointer. */
int imgxf_permute_u8(const imgxf_view* src, const imgxf_view* dst, const int32_t* perm,
                     void* stream);
/* Image.composite(im1, im2, mask) transformation.py:344 for a 0/255 mask (c==1): mask ? im1 : im2. */
int imgxf_composite_u8(const imgxf_view* im1, const imgxf_view* im2, const imgxf_view* mask,
                       const imgxf_view* dst, void* stream);
/* Image.composite(im1, Image.new(mode, size, colour), mask) without materialising the constant image
 * (transformation.py:333,344). */
int imgxf_composite_const_u8(const imgxf_view* im1, const uint8_t* colour, const imgxf_view* mask,
                             const imgxf_view* dst, void* stream);

/* ---- Image.filter(ImageFilter.Kernel((3,3), kernel, scale, offset)) — libImaging ImagingFilter3x3
 * (ImageFilter.SMOOTH behind ImageEnhance.Sharpness, cifar_image_transformations.py:95-99):
 * float32 coefficients kernel9[i]/scale (HOST pointer, Pillow's order: first triple = row y+1),
 * ss = offset + 0.5 then one (a*k0 + b*k1) + c*k2 per row, clip8 truncation; the one-pixel
 * frame of the image is copied from the input.  Any c. */
int imgxf_filter3x3_u8(const imgxf_view* src, const imgxf_view* dst, const float* kernel9,
                       float scale, float offset, void* stream);

/* ---- TransformationPool noise members, device half (cifar_image_transformations.py:39-70) ------
 * The random draws stay on the host with NumPy's generator, exactly as the reference makes them;
 * these apply them.  All float views are float64 (8-byte aligned).
 * add_noise_f64:  dst = trunc(clip(f64(f32(p)) + noise, 0, 255))                   (:45-47)
 * shot_noise:     dst = trunc(clip(counts / lambda * 255.0, 0, 255)), counts = Poisson draws (:68-69)
 * impulse_noise:  mask [n,h,w,1]: mask < lo -> 0, mask > hi -> 255, else src      (:57-58) */
int imgxf_add_noise_f64_u8(const imgxf_view* src, const imgxf_view* noise_f64, const imgxf_view* dst, void* stream);
int imgxf_shot_noise_u8(const imgxf_view* counts_f64, double lambda, const imgxf_view* dst, void* stream);
int imgxf_impulse_noise_u8(const imgxf_view* src, const imgxf_view* mask_f64, double lo, double hi,
                           const imgxf_view* dst, void* stream);

/* ---- AugMix point ops and histograms  fall_2025/AugMix.py:31,36,37; Initial_Experiments.py:95-113
 * lut:       dst = lut[channel][src], lut = host table of c*256 bytes (ImageOps.posterize /
 *            solarize / any Image.point table); copied into the launch, no device allocation.
 * equalize:  ImageOps.equalize per frame and channel (histogram -> table -> map), all on the
 *            device.  workspace: >= n*c*256*5 bytes, 4-byte aligned.
 * channel_histogram: hist[n][c][256] uint32 (device, zeroed by the call) of an interleaved view. */
int imgxf_lut_u8(const imgxf_view* src, const imgxf_view* dst, const uint8_t* lut, void* stream);
int imgxf_equalize_u8(const imgxf_view* src, const imgxf_view* dst, void* workspace, size_t workspace_bytes,
                      void* stream);
int imgxf_channel_histogram_u8(const imgxf_view* src, uint32_t* hist, void* stream);

/* ---- AugMix on a batch  fall_2025/AugMix.py:45-62 -------------------------------------------
 * One launch runs augmix() for n float CHW images: per image `width` branches of operations on
 * uint8 HWC frames, then the float32 mix, bit-identical to imagetransformations_amd.augmix.augmix().
 *
 * Operation table (HOST, copied into the launch): at most IMGXF_AUGMIX_MAX_OPS entries.
 *   IDENTITY  no operation (Image.rotate by a multiple of 360 degrees);
 *   QUARTER   arg = counter-clockwise quarter turns 1..3 (1 and 3 need h == w; imgxf_rot90_u8);
 *   AFFINE    NEAREST Image.transform(AFFINE, m), fill 0, libImaging affine_fixed 16.16 (imgxf_affine_u8);
 *   SCALE     NEAREST with m[1] == m[3] == 0, fill 0, ImagingScaleAffine (imgxf_affine_scale_nearest_u8);
 *   LUT       dst = luts[arg][src] on every channel (ImageOps.posterize / solarize tables);
 *   EQUALIZE  ImageOps.equalize per channel (imgxf_equalize_u8).
 * m[6] is the destination->source matrix as Pillow takes it (AFFINE and SCALE; ignored otherwise).
 * luts: HOST, nluts * 256 bytes, nluts <= IMGXF_AUGMIX_MAX_LUTS.
 *
 * plan (DEVICE, 4-byte aligned): n records of imgxf_augmix_record_bytes(width, depth) bytes each:
 *   float   w[width]            branch weights, (float) of the Dirichlet draw
 *   float   one_minus_m, m      (float)(1 - m) with 1 - m formed in double, and (float) m
 *   uint8_t step[width][depth]  operation-table index of each step; indices >= nops end nothing and
 *                               run nothing (0xFF marks the steps past a branch's drawn depth)
 * src: n float CHW images in [0, 1] at element strides strides[0..3] (image, channel, row, column);
 * dst: contiguous float [n][3][h][w], must not overlap src.
 * workspace (DEVICE, 16-byte aligned): imgxf_augmix_workspace_bytes(n, h, w) bytes.  It is 0 when
 * the two uint8 working frames stay in LDS, i.e. when
 *     2 * R16(3*h*w) + R16(4*(h + w + 2)) + 4992 <= 163840   (R16 = round up to 16),
 * which admits every square frame up to 162 x 162; otherwise 2 * R16(3*h*w) * n bytes hold the
 * working frames of every image and the same kernel runs on them.
 * Errors: IMGXF_ERR_NULL (strides, ops; src, dst, plan when n > 0; luts when nluts > 0; a NULL workspace of
 * sufficient workspace_bytes when one is needed),
 * IMGXF_ERR_SHAPE (h, w outside 1..32767, n < 0), IMGXF_ERR_ARG (unknown op code, an arg outside its
 * range, a non-finite matrix entry, nops / nluts / width / depth out of range),
 * IMGXF_ERR_WORKSPACE (workspace_bytes short).  All checks happen on the host before any HIP call. */
enum { IMGXF_AUGMIX_IDENTITY = 0, IMGXF_AUGMIX_QUARTER = 1, IMGXF_AUGMIX_AFFINE = 2, IMGXF_AUGMIX_SCALE = 3,
       IMGXF_AUGMIX_LUT = 4, IMGXF_AUGMIX_EQUALIZE = 5 };
enum { IMGXF_AUGMIX_MAX_OPS = 16, IMGXF_AUGMIX_MAX_LUTS = 4, IMGXF_AUGMIX_MAX_WIDTH = 1024,
       IMGXF_AUGMIX_MAX_DEPTH = 1024 };
typedef struct imgxf_augmix_op {
    int32_t code;   /* IMGXF_AUGMIX_* */
    int32_t arg;    /* QUARTER: turns; LUT: table index; 0 otherwise */
    double  m[6];
} imgxf_augmix_op;
/* Bytes of one plan record: 4 * width + 8 + width * depth, rounded up to a multiple of 4. */
int imgxf_augmix_record_bytes(int32_t width, int32_t depth, size_t* bytes);
int imgxf_augmix_workspace_bytes(int32_t n, int32_t h, int32_t w, size_t* bytes);
int imgxf_augmix_f32(const float* src, int32_t n, int32_t h, int32_t w, const int64_t* strides, float* dst,
                     const imgxf_augmix_op* ops, int32_t nops, const uint8_t* luts, int32_t nluts,
                     const void* plan, int32_t width, int32_t depth, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---- TransformationPool chains on a batch  cifar_image_transformations.py:37-129,141-152 ------
 * One launch runs a chain of TransformationPool members on each of n RGB uint8 frames, bit-identical
 * to the per-image members of imagetransformations_amd.pool (one or two launches per member each).
 *
 * Operation table (HOST, copied into the launch): at most IMGXF_POOL_MAX_OPS entries.
 *   DEFOCUS_BLUR        m[0] = GaussianBlur radius (as a float); 3 + 3 box passes with the box radius
 *                       of imgxf_gaussian_blur_pil_u8;
 *   ENHANCE_SHARPNESS   m[0..8] = 3x3 kernel, m[9] = scale (ImageFilter.SMOOTH: ImagingFilter3x3,
 *                       border pixels copied), then the blend with the frame by the step's factor;
 *   ENHANCE_CONTRAST    blend with the frame's solid int(mean(L) + 0.5) by the step's factor;
 *   ENHANCE_COLOR       blend with convert('L') replicated to RGB by the step's factor;
 *   ENHANCE_BRIGHTNESS  blend with black by the step's factor;
 *   GAUSSIAN_NOISE      trunc(clip(f64(p) + z, 0, 255)), z = the step's float64 [h][w][3] slice;
 *   IMPULSE_NOISE       m[0] = lo, m[1] = hi: mask < lo -> 0, mask > hi -> 255, mask = the step's
 *                       float64 [h][w] slice;
 *   SHOT_NOISE          m[0] = lambda > 0: trunc(clip(k / lambda * 255, 0, 255)), k = the step's float64
 *                       [h][w][3] slice of Poisson counts (the frame itself is not read);
 *   MOTION_BLUR         arg = size, odd, 1..31: one row of (float)(1/size) taps, REFLECT_101, rounded;
 *   HISTOGRAM_EQUALIZATION  RGB -> YUV, cv2.equalizeHist on Y, YUV -> RGB (imgxf_rgb2yuv_u8 ...).
 * Blends are Blend.c's float32 in1 + factor * (in2 - in1), truncated, clipped outside [0, 1].
 *
 * plan (DEVICE, 8-byte aligned): n records of imgxf_pool_chain_record_bytes(steps) bytes; step s is
 *   uint8_t  op          operation-table index; indices >= nops run nothing
 *   uint8_t  pad[3]
 *   float    factor      the blend factor of the ENHANCE_* ops (the C float of the member's argument)
 *   uint64_t offset      byte offset into payload of the step's float64 slice (noise ops; 8-aligned);
 *                        a slice that does not lie inside payload_bytes runs nothing
 * payload (DEVICE, 8-byte aligned, may be NULL when payload_bytes is 0): the noise ops' float64 data.
 * src: n RGB frames (c == 3), any row and frame stride; dst: same geometry, must not overlap src.
 * workspace (DEVICE, 16-byte aligned): imgxf_pool_chain_workspace_bytes(n, h, w) bytes.  It is 0
 * when the two uint8 working frames stay in LDS, i.e. when
 *     2 * R16(3*h*w) + 1344 <= 163840   (R16 = round up to 16),
 * which admits every square frame up to 164 x 164; otherwise 2 * R16(3*h*w) * n bytes hold the
 * working frames of every image and the same kernel runs on them.
 * Errors: IMGXF_ERR_NULL (src, dst, ops; plan when n > 0; payload when payload_bytes > 0; a NULL
 * workspace of sufficient workspace_bytes when one is needed), IMGXF_ERR_SHAPE (a bad view, c != 3,
 * src and dst geometry differ), IMGXF_ERR_ARG (unknown op code, an argument outside its range,
 * nops or steps out of range, a misaligned plan, payload or workspace), IMGXF_ERR_WORKSPACE
 * (workspace_bytes short).  All checks happen on the host before any HIP call. */
enum { IMGXF_POOL_DEFOCUS_BLUR = 0, IMGXF_POOL_ENHANCE_SHARPNESS = 1, IMGXF_POOL_ENHANCE_CONTRAST = 2,
       IMGXF_POOL_ENHANCE_COLOR = 3, IMGXF_POOL_ENHANCE_BRIGHTNESS = 4, IMGXF_POOL_GAUSSIAN_NOISE = 5,
       IMGXF_POOL_IMPULSE_NOISE = 6, IMGXF_POOL_SHOT_NOISE = 7, IMGXF_POOL_MOTION_BLUR = 8,
       IMGXF_POOL_HISTOGRAM_EQUALIZATION = 9 };
enum { IMGXF_POOL_MAX_OPS = 32, IMGXF_POOL_MAX_STEPS = 16, IMGXF_POOL_MAX_MOTION = 31 };
typedef struct imgxf_pool_op {
    int32_t code;   /* IMGXF_POOL_* */
    int32_t arg;    /* MOTION_BLUR: size; 0 otherwise */
    double  m[10];
} imgxf_pool_op;
/* Bytes of one plan record: 16 * steps, steps in 1..IMGXF_POOL_MAX_STEPS. */
int imgxf_pool_chain_record_bytes(int32_t steps, size_t* bytes);
int imgxf_pool_chain_workspace_bytes(int32_t n, int32_t h, int32_t w, size_t* bytes);
int imgxf_pool_chain_u8(const imgxf_view* src, const imgxf_view* dst, const imgxf_pool_op* ops, int32_t nops,
                        const void* plan, int32_t steps, const void* payload, size_t payload_bytes,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- TransformationPool chains on a LIST of frames of any sizes ---------------------------------
 * The same chains, one workgroup per frame, on frames that each have their own size, source and
 * place in one output allocation; the steps are the statements of imgxf_pool_chain_u8 (one device
 * body, csrc/pool_chain_steps.inc), so a frame's bytes are those of a batch of its size.
 *
 * Frame record (56 bytes).  The caller writes n of them once, into the block it copies to the device
 * (with the step records and the host-drawn payload: one host-to-device copy), and hands the HOST
 * copy as `frames` — every check reads that one — and the place of the device copy as
 * block + frames_off.  The two copies must hold the same bytes. */
typedef struct imgxf_pool_list_frame {
    uint64_t src;         /* DEVICE address of the frame's first byte; RGB uint8, pixels of a row dense */
    int64_t  src_stride;  /* bytes from one row to the next, >= 3 * w */
    uint64_t out_off;     /* byte offset in out of the frame's contiguous [h][w][3] result; 16-aligned */
    uint64_t ws_off;      /* byte offset in workspace of its 2 * R16(3*h*w) working bytes; 16-aligned;
                             read only for a frame that is not resident */
    uint64_t rec_off;     /* byte offset in block of its `steps` step records (16 bytes each, as the
                             plan of imgxf_pool_chain_u8; their payload offsets count from payload); 8-aligned */
    int32_t  h, w;        /* 1..32767, 3*h*w <= 0x7fffff00 */
    int32_t  steps;       /* 0..IMGXF_POOL_MAX_STEPS; 0 copies the frame */
    int32_t  pad_;
} imgxf_pool_list_frame;
/* A frame's launch class, the dynamic LDS it needs and its workspace bytes.  Resident frames (the
 * bound of imgxf_pool_chain_u8) fall into classes 0, 1, 2 by LDS need: up to 52 KiB (three
 * workgroups per CU, all that the kernel's registers admit), up to 80 KiB (two per CU), up to
 * 160 KiB (one); workspace_bytes is 0.  Every other frame is of class 3: lds_bytes is the fixed 1344 and
 * workspace_bytes 2 * R16(3*h*w).  IMGXF_ERR_SHAPE outside the limits above. */
enum { IMGXF_POOL_LIST_CLASSES = 4 };
int imgxf_pool_chain_list_class(int32_t h, int32_t w, int32_t* cls, size_t* lds_bytes, size_t* workspace_bytes);
/* One launch per class present, at most IMGXF_POOL_LIST_CLASSES, whatever n and the number of
 * distinct sizes: the records must come sorted by class (ascending), and a launch declares the LDS
 * of the largest frame in it.  ops / nops / payload: as imgxf_pool_chain_u8.  block (DEVICE,
 * 8-aligned, block_bytes): holds the frame records at frames_off (8-aligned) and the step records.
 * out (DEVICE, 16-aligned, out_bytes), workspace (DEVICE, 16-aligned; may be NULL when no frame
 * needs one).  Outputs must not overlap each other, any source, or another frame's working bytes.
 * Errors, all found on the host before any launch: IMGXF_ERR_NULL (ops; frames, block or out when
 * n > 0; payload when payload_bytes > 0; a frame's src; workspace when a frame needs it),
 * IMGXF_ERR_SHAPE (n < 0, a frame's h, w or src_stride), IMGXF_ERR_ARG (the operation table, nops,
 * a frame's steps, a misaligned pointer or offset, records or an output outside block / out,
 * records not sorted by class), IMGXF_ERR_WORKSPACE (a frame's working bytes outside workspace). */
int imgxf_pool_chain_list_u8(const imgxf_pool_list_frame* frames, int32_t n, const imgxf_pool_op* ops, int32_t nops,
                             const void* block, size_t block_bytes, size_t frames_off,
                             const void* payload, size_t payload_bytes, void* out, size_t out_bytes,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- TransformationPool.histogram_equalization  cifar_image_transformations.py:122-129 -------
 * cv2.cvtColor(RGB2YUV / YUV2RGB) for 8-bit images (integer BT.601, yuv_shift 14) and
 * cv2.equalizeHist applied to one channel of an interleaved view.  PARITY UNPINNED: OpenCV is not
 * installed in the build container; the arithmetic follows OpenCV's integer definitions.
 * workspace of equalize_hist_cv: >= n*c*256*5 bytes, 4-byte aligned. */
int imgxf_rgb2yuv_u8(const imgxf_view* src, const imgxf_view* dst, void* stream);
int imgxf_yuv2rgb_u8(const imgxf_view* src, const imgxf_view* dst, void* stream);
int imgxf_equalize_hist_cv_u8(const imgxf_view* src, const imgxf_view* dst, int channel, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- ImageFilter.BoxBlur / ImageFilter.GaussianBlur — libImaging BoxBlur.c --------------------
 * (TransformationPool.defocus_blur, cifar_image_transformations.py:72-77.)  `passes` box passes
 * along x then along y, each in exact uint32 arithmetic with replicated edges and a uint8
 * intermediate.  workspace: device scratch of n*h*w*c bytes (needed when more than one pass
 * runs).  gaussian_blur_pil: box radius from Pillow's _gaussian_blur_radius, 3 passes. */
int imgxf_box_blur_u8(const imgxf_view* src, const imgxf_view* dst, float xradius, float yradius,
                      int passes, void* workspace, size_t workspace_bytes, void* stream);
int imgxf_gaussian_blur_pil_u8(const imgxf_view* src, const imgxf_view* dst, float radius,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- ImageEnhance.Color / .Contrast ---------------------------------
 * pipenline/cifar_image_transformations.py:81-85,102-106.  Both are Image.blend(degenerate,
 * image, factor) with the Blend.c float semantics above.
 * Color: degenerate = convert('L') replicated to RGB (fused per pixel).  c == 3.
 * Contrast: degenerate = solid int(mean(L) + 0.5) per frame; `sums` is device scratch of n
 * uint64 (zeroed by the call) that receives every frame's sum of L.  c in {1,3}. */
int imgxf_enhance_color_u8(const imgxf_view* src, const imgxf_view* dst, float factor, void* stream);
int imgxf_enhance_contrast_u8(const imgxf_view* src, const imgxf_view* dst, float factor,
                              uint64_t* sums, void* stream);

/* ---- crop / paste / fill (Image.crop, Image.paste, Image.new) transformation.py:187-193,287-305 */
/* Fill every pixel of dst with color[c] (HOST pointer). */
int imgxf_fill_u8(const imgxf_view* dst, const uint8_t* color, void* stream);
/* Copy the rectangle (sx,sy,rw,rh) of src to (dx,dy) of dst for every frame (same n, c). */
int imgxf_copy_rect_u8(const imgxf_view* src, const imgxf_view* dst, int sx, int sy, int dx,
                       int dy, int rw, int rh, void* stream);
/* apply_translation (transformation.py:284-307: Image.new(black) + crop + paste) in one pass:
 * dst(x, y) = src(x - dx, y - dy) where that pixel exists, else fill[c] (HOST pointer).  Same n,h,w,c. */
int imgxf_translate_u8(const imgxf_view* src, const imgxf_view* dst, int dx, int dy,
                       const uint8_t* fill, void* stream);
/* Image.transpose(ROTATE_90/180/270) fast paths of Image.rotate (PIL/Image.py:2513-2521).
 * quarter_turns_ccw in {1,2,3}. */
int imgxf_rot90_u8(const imgxf_view* src, const imgxf_view* dst, int quarter_turns_ccw,
                   void* stream);
/* Image.transpose(FLIP_LEFT_RIGHT) (mode 0; vert_flip, fall_2025/transformations_code:39-41) or
 * FLIP_TOP_BOTTOM (mode 1).  Same geometry in and out. */
int imgxf_flip_u8(const imgxf_view* src, const imgxf_view* dst, int mode, void* stream);

/* ---- float-tensor corruption maps  pipenline/angellic.py:34-46, angellic2.py:47-50 -------*/
/* Unnormalised fp32 images in [0,1], any shape, `count` contiguous elements (device pointers,
 * 4-byte aligned; in-place allowed).  mode BRIGHTNESS: clamp(x + p0, 0, 1); CONTRAST:
 * clamp((x - 0.5)*p0 + 0.5, 0, 1); NOISE: clamp(x + (noise*p0 + p1), 0, 1) with `noise` the
 * caller's torch.randn_like draw (std = p0, mean = p1).  Same fp32 operations in the same order as
 * torch's eager kernels (bit-identical).  mask (optional, device, `count` bytes): 1 where the
 * value before the clamp lay in [0,1], i.e. where torch.clamp's backward passes the gradient. */
enum { IMGXF_F32_BRIGHTNESS = 0, IMGXF_F32_CONTRAST = 1, IMGXF_F32_NOISE = 2 };
int imgxf_f32_map(const float* src, const float* noise, float* dst, uint8_t* mask, int64_t count,
                  int mode, float p0, float p1, void* stream);

/* transforms.ToTensor() (+ transforms.Normalize(mean, std)): uint8 HWC frames -> float32
 * [n][c][h][w] planes at `dst` (device, contiguous), x/255 correctly rounded, then
 * (x - mean[c]) / std[c] in fp32 — bit-identical to torchvision's tensor arithmetic.  mean / std:
 * HOST float[c], both NULL = ToTensor only.  c in {1,3,4}. */
int imgxf_to_tensor_f32(const imgxf_view* src, float* dst, const float* mean, const float* std,
                        void* stream);

/* ---- perspective warp  fall_2025/transformations_code:54-66 -----------------------------*/
/* torchvision RandomPerspective on a float tensor for given coefficients: ToTensor (u8/255),
 * _perspective_grid + grid_sample(bilinear, padding zeros, align_corners=False) of the image and
 * a ones channel, img*mask + (1-mask)*0, ToPILImage (mul(255).byte()), all in fp32 in the
 * evaluation order of the torch CPU build.  coeffs: HOST float[8] (per_frame = 0, shared by
 * all frames) or float[n][8] (per_frame = 1), as returned by torchvision's
 * _get_perspective_coeffs (output pixel -> source).  src and dst have the same n, h, w, c
 * (c in {1,3,4}) and must not alias. */
int imgxf_perspective_bilinear_u8(const imgxf_view* src, const imgxf_view* dst,
                                  const float* coeffs, int per_frame, void* stream);
/* HOST only, no device: what the kernel decides for the 64 x 16 output tile at (tx0, ty0) (multiples of 64 and 16 inside
 * the frame) of a w x h x c frame (w, h <= 32767, c in {1,3,4}) with coeffs float[8]; src_dwords: 1 where the source is
 * staged as aligned dwords (base, row and frame stride multiples of 4, a frame below 4 GiB), else 0.
 * out[8] = staged (the tile's source box goes to LDS; 0: the taps are gathered from global memory), interior (every tap
 * is read from the box unchecked), bx0, by0, bw, bh (the box; bw = bh = 0: the tile sees no source pixel), pitch (floats
 * per staged row), gb0 (first staged byte of a source row).  The same function as the kernel's first wave evaluates. */
int imgxf_perspective_tile_plan_host(int w, int h, int c, int src_dwords, const float* coeffs, int tx0, int ty0, int* out);

/* ---- the driver's save step  transformation.py:161-162 (`transformed.save(path)`: Pillow ->
 * libjpeg-turbo baseline JPEG, 4:2:0, islow DCT, no restart markers) ------------------------*/
typedef struct imgxf_jpeg_tables {
    uint16_t quant[2][64];      /* luminance / chrominance divisors 1..255, natural (row-major) order */
    uint16_t dc_code[2][16];    /* Huffman code of DC magnitude category 0..11 (table 0: Y, 1: Cb/Cr) */
    uint8_t  dc_len[2][16];
    uint16_t ac_code[2][256];   /* Huffman code of the AC symbol (run << 4) | size */
    uint8_t  ac_len[2][256];
} imgxf_jpeg_tables;
/* One complete JPEG file per frame of a c == 3 view: out + f*out_frame_stride holds `header`
 * (host bytes, SOI .. SOS as the caller built them for these tables and this size, <= 1024),
 * the entropy-coded segment, EOI; sizes[f] (device) = the file's length, or 0xFFFFFFFF when it
 * does not fit in out_frame_stride bytes (nothing usable is written for that frame).
 * Bit-identical to libjpeg(-turbo)'s output for the same tables.  workspace: device, 16-byte
 * aligned, >= imgxf_jpeg_workspace_bytes(n, h, w, out_frame_stride).  Limits: n <= 65535,
 * out_frame_stride <= 2^31, ceil(w/16)*ceil(h/16) < 349525 MCUs per frame (bit offsets are
 * 32-bit; 8K frames fit), else IMGXF_ERR_SHAPE / IMGXF_ERR_ARG. */
int imgxf_jpeg_workspace_bytes(int n, int h, int w, size_t out_frame_stride, size_t* bytes);
int imgxf_jpeg_encode_u8(const imgxf_view* src, const imgxf_jpeg_tables* tables, const uint8_t* header,
                         int header_bytes, uint8_t* out, size_t out_frame_stride, uint32_t* sizes,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The same default file (RGB, 4:2:0, the call's tables, one quality per call) for a LIST of frames of different sizes,
 * in a number of launches that does not depend on the list: every stage of imgxf_jpeg_encode_u8 runs once over work-unit
 * tables instead of over a (items, frames) grid.  The HOST lays out one block
 *     imgxf_jpeg_list_header | imgxf_jpeg_list_frame[n] | imgxf_jpeg_list_unit tables (5)
 * which the caller completes (data, row_stride of every frame) and copies to the device once.  Each frame has its own
 * geometry, its own piece of every workspace area, its own 32-bit bit offsets and its own slot of the output. */
#define IMGXF_JPEG_LIST_STAGES 5    /* unit tables: 16x256-pixel transform strips (item = strip | MCU row << 16), groups of
                                       256 blocks, scan parts of 1024 blocks, chunk groups, scan parts of 1024 chunks */
#define IMGXF_JPEG_LIST_AREAS 8     /* workspace areas: coefficients, DC values, AC bits, lens / bit offsets, partial sums,
                                       totals (bits[n], 0xFF counts[n]), unstuffed streams, 0xFF counts per 32-byte chunk */
typedef struct imgxf_jpeg_list_header {
    int32_t  n_frames, frames_off, total_bytes, pad_;       /* byte offsets into the block; its size */
    int32_t  n_units[IMGXF_JPEG_LIST_STAGES], units_off[IMGXF_JPEG_LIST_STAGES];
    uint64_t area_off[IMGXF_JPEG_LIST_AREAS];                /* byte offsets into the workspace, 256-byte aligned */
    uint64_t workspace_bytes, out_bytes;
} imgxf_jpeg_list_header;
typedef struct imgxf_jpeg_list_frame {
    uint64_t data;              /* DEVICE address of pixel (0, 0), any alignment; filled by the caller, as is row_stride */
    int64_t  row_stride;        /* bytes, >= 3 w */
    int32_t  h, w;
    int32_t  mw, mh, bw, bh, nblk;   /* MCUs (16x16) and blocks (8x8) across / down; 6 mw mh blocks */
    int32_t  nparts_blk, nchunks, nparts_chunk, chunk_groups;   /* scan parts of the blocks; 32-byte chunks of the stream,
                                   their scan parts, the workgroups (<= 256) that share them */
    int32_t  pad_;
    int64_t  stream_words;      /* capacity of the unstuffed stream: out_cap / 4 rounded up, + 4, to a multiple of 4 */
    int64_t  coef_off, blk_off, part_off, stream_off, cnt_off;   /* the frame's ELEMENT offset in its areas: int16
                                   coefficients (whole groups of 64 blocks); blocks (a multiple of 64: the DC, AC-bits and
                                   lens areas share it); uint32 partial sums; uint32 stream words (a multiple of 4); chunks */
    int64_t  out_off, out_cap;  /* the file's slot of `out`: byte offset (a multiple of 16) and capacity */
} imgxf_jpeg_list_frame;
typedef struct imgxf_jpeg_list_unit {
    int32_t frame, item;        /* one workgroup: item `item` of frame `frame` (frame-major, items ascending) */
} imgxf_jpeg_list_unit;
/* HOST half (no device work).  sizes: int32 [n][2] = (h, w); capacities: n file capacities in bytes (out_cap).  Writes the
 * block (block == NULL: the sizes only) and reports the block's bytes (the tables), the workspace's and the output's.
 * The workspace never exceeds the sum over the frames of imgxf_jpeg_workspace_bytes(1, h, w, capacity).
 * Errors: IMGXF_ERR_NULL; IMGXF_ERR_SHAPE for n < 0 or n > 1048576, h or w outside 1..32767, more than 2097143 blocks in
 * a frame; IMGXF_ERR_ARG for a capacity below 1024 + 2 or above 2^31, a block over 2 GiB; IMGXF_ERR_WORKSPACE when
 * block_cap is too small. */
int imgxf_jpeg_encode_list_layout_host(const int32_t* sizes, const uint64_t* capacities, int n, void* block, size_t block_cap,
                                       size_t* block_bytes, size_t* workspace_bytes, size_t* out_bytes);
/* The launches: block_host is the caller's host copy of the block, block_dev the same bytes on the device (8-byte
 * aligned).  `header` is the file header for these tables with ANY size in its SOF0 segment: the device writes each
 * frame's height and width there.  File f goes to out + frames[f].out_off; sizes[f] (device, n entries) as
 * imgxf_jpeg_encode_u8.  Every record is checked on the host before anything is launched: the block must be what
 * imgxf_jpeg_encode_list_layout_host writes for the records' (h, w, out_cap) — so offsets are aligned, ascending,
 * disjoint and inside the workspace and `out`, and every block of every frame belongs to exactly one unit — else
 * IMGXF_ERR_ARG; a NULL data -> IMGXF_ERR_NULL; h, w, row_stride < 3 w or the block limit -> IMGXF_ERR_SHAPE; a
 * workspace or `out` too small or misaligned (16 bytes) -> IMGXF_ERR_WORKSPACE; a header without SOF0 -> IMGXF_ERR_ARG. */
int imgxf_jpeg_encode_list_u8(const void* block_host, const void* block_dev, const imgxf_jpeg_tables* tables,
                              const uint8_t* header, int header_bytes, uint8_t* out, size_t out_bytes, uint32_t* sizes,
                              void* workspace, size_t workspace_bytes, void* stream);

/* The writer's options: Pillow's `save(fp, "JPEG", quality=q, subsampling=s, optimize=o)` for RGB (ncomp 3, a c == 3 view)
 * and "L" frames (ncomp 1, c == 1), bit-identical to libjpeg-turbo.  Luma sampling h_samp x v_samp: 1x1 (4:4:4, MCU 8x8:
 * Y Cb Cr; jcsample.c fullsize_downsample), 2x1 (4:2:2, MCU 16x8: Y Y Cb Cr; h2v1_downsample, bias 0,1 along a row, dummy
 * luma blocks when ceil(w/8) is odd), 2x2 (4:2:0, the file of imgxf_jpeg_encode_u8).  A grayscale frame is one
 * non-interleaved component, one block per MCU whatever its sampling: h_samp / v_samp then only reach the SOF the caller
 * writes.  Rows / columns past the image repeat the last one (expand_right_edge, jcprepct.c); dummy blocks carry zero AC
 * and the DC of the block before them (jccoefct.c).
 * optimize = 1: per frame, the symbol counts of every block (jchuff.c htest_one_block, dummy blocks included; table 1 shared
 * by Cb and Cr), jpeg_gen_optimal_table (code point 256 reserved, ties to the larger symbol, 16-bit limit) and
 * jpeg_make_c_derived_tbl; the device then writes the frame's DHT segments (DC0, AC0[, DC1, AC1]) and SOS after `header`,
 * which is then SOI .. SOF only, and only the quantisers of `tables` are read.  Without optimize `header` is SOI .. SOS
 * for the Huffman tables in `tables`.  4:2:0 without optimize is imgxf_jpeg_encode_u8 itself.
 * Errors as imgxf_jpeg_encode_u8, plus: c != ncomp -> IMGXF_ERR_UNSUPPORTED; ncomp, sampling or optimize out of range, a
 * quantiser of a used table outside 1..255, header_bytes outside 2..1024 -> IMGXF_ERR_ARG.  Bit offsets are 32-bit: at most
 * 2097143 blocks per frame — ceil(w/16)*ceil(h/16) < 349525 MCUs at 4:2:0 (6 blocks each), < 524287 at 4:2:2 (16x8, 4
 * blocks), ceil(w/8)*ceil(h/8) < 699047 at 4:4:4 (3 blocks: twice the chroma blocks of 4:2:0) and < 2097143 grayscale;
 * past it IMGXF_ERR_SHAPE.  With optimize, a frame whose optimal Huffman table would need a code longer than 32 bits
 * (libjpeg's JERR_HUFF_CLEN_OVERFLOW: ~15 M symbols in Fibonacci-shaped counts) gets sizes[f] = 0xFFFFFFFE and no file. */
typedef struct imgxf_jpeg_enc_params {
    int32_t ncomp;              /* 1 (grayscale) or 3 (YCbCr from RGB) */
    int32_t h_samp, v_samp;     /* luma sampling: 1x1, 2x1 or 2x2 */
    int32_t optimize;           /* 0: the Huffman tables of `tables`; 1: per-frame optimal tables */
} imgxf_jpeg_enc_params;
int imgxf_jpeg_workspace_bytes_ex(const imgxf_jpeg_enc_params* params, int n, int h, int w, size_t out_frame_stride,
                                  size_t* bytes);
/* The optimize path's table stage alone (jchuff.c jpeg_gen_optimal_table + jpeg_make_c_derived_tbl), for n frames of
 * four tables each (DC0, AC0, DC1, AC1).  Device pointers: counts uint32[n][4][256] (symbol counts); dht [n][4] records of
 * 276 bytes — uint32 nvals (0xFFFFFFFF: a code would exceed 32 bits), BITS[16], HUFFVAL[256]; codes uint32[n][544] —
 * code | length << 16 of DC tables 0, 1 (16 symbols each), then AC tables 0, 1 (256 each). */
int imgxf_jpeg_optimal_tables(const uint32_t* counts, int n, uint8_t* dht, uint32_t* codes, void* stream);
int imgxf_jpeg_encode_ex_u8(const imgxf_view* src, const imgxf_jpeg_enc_params* params, const imgxf_jpeg_tables* tables,
                            const uint8_t* header, int header_bytes, uint8_t* out, size_t out_frame_stride,
                            uint32_t* sizes, void* workspace, size_t workspace_bytes, void* stream);

/* The list writer for every sequential class of imgxf_jpeg_encode_ex_u8: one call writes a LIST of frames of different
 * sizes that share one class (ncomp, sampling, optimize) — 4:4:4, 4:2:2, 4:2:0 or grayscale, with the call's tables or each
 * frame's own optimal ones — in a number of launches that depends on the class alone, never on the list.  A grayscale
 * class is stated as 1x1 (h_samp / v_samp reach only the SOF the caller writes).  The block is
 *     imgxf_jpeg_list_ex_header | imgxf_jpeg_list_frame[n] | imgxf_jpeg_list_unit tables (5)
 * with the records and unit tables of imgxf_jpeg_encode_list_u8, laid out for the class: MCUs of 8x8 (4:4:4, grayscale),
 * 16x8 (4:2:2) or 16x16 pixels and 3, 1, 4 or 6 blocks; row_stride >= ncomp * w; the transform units (stage 0) are
 * 16x256-pixel strips at 4:2:0 and one MCU row of 512 pixels in the other layouts (item = strip | MCU row << 16).  With
 * optimize three more workspace areas, indexed by the frame, hold what imgxf_jpeg_optimal_tables describes: symbol counts
 * uint32 [n][4][256] (zeroed by the call, in stream order), code words uint32 [n][544], DHT records [n][4] of 276 bytes;
 * without it they are empty, at the workspace's end.  For {3, 2, 2, 0} frames, units and sizes are those of
 * imgxf_jpeg_encode_list_layout_host and the files those of imgxf_jpeg_encode_list_u8. */
#define IMGXF_JPEG_LIST_OPT_AREAS 3
typedef struct imgxf_jpeg_list_ex_header {
    imgxf_jpeg_list_header list;                             /* frames_off = sizeof(imgxf_jpeg_list_ex_header) */
    imgxf_jpeg_enc_params  params;                           /* the class the block was laid out for */
    uint64_t opt_off[IMGXF_JPEG_LIST_OPT_AREAS];             /* byte offsets into the workspace, 256-byte aligned */
} imgxf_jpeg_list_ex_header;
/* HOST half, as imgxf_jpeg_encode_list_layout_host.  The workspace never exceeds the sum over the frames of
 * imgxf_jpeg_workspace_bytes_ex(params, 1, h, w, capacity).  Errors as there, plus IMGXF_ERR_ARG for params outside the
 * classes above (ncomp, sampling, optimize; grayscale not 1x1) and IMGXF_ERR_SHAPE for more than 65535 frames with optimize
 * (the table stage runs one workgroup per table and frame). */
int imgxf_jpeg_encode_list_ex_layout_host(const imgxf_jpeg_enc_params* params, const int32_t* sizes, const uint64_t* capacities,
                                          int n, void* block, size_t block_cap, size_t* block_bytes, size_t* workspace_bytes,
                                          size_t* out_bytes);
/* The launches, as imgxf_jpeg_encode_list_u8: `header` is SOI .. SOS for the class (any size in SOF0) or, with optimize,
 * SOI .. SOF0 — the device then writes, into the frame's slot, that prefix with the frame's own height and width, the
 * frame's DHT segments and SOS, its stuffed data and EOI.  sizes[f] as imgxf_jpeg_encode_ex_u8: the file's length,
 * 0xFFFFFFFF when it does not fit out_cap (the slot is then untouched past that bound), 0xFFFFFFFE when an optimal table
 * would need a code over 32 bits.  The same checks in the same order as imgxf_jpeg_encode_list_u8, all of the block's
 * before a device pointer is looked at; a block laid out for other params -> IMGXF_ERR_ARG. */
int imgxf_jpeg_encode_list_ex_u8(const void* block_host, const void* block_dev, const imgxf_jpeg_enc_params* params,
                                 const imgxf_jpeg_tables* tables, const uint8_t* header, int header_bytes, uint8_t* out,
                                 size_t out_bytes, uint32_t* sizes, void* workspace, size_t workspace_bytes, void* stream);

/* Progressive files: Pillow's `save(fp, "JPEG", progressive=True, quality=q, subsampling=s)` for the frames and layouts of
 * imgxf_jpeg_encode_ex_u8, bit-identical to libjpeg-turbo.  The coefficients are the sequential writer's; the file is
 * jcparam.c jpeg_simple_progression (colour, 10 scans: Y Cb Cr DC 0-0 Al 1; Y 1-5 Al 2; Cr, Cb 1-63 Al 1; Y 6-63 Al 2;
 * Y 1-63 Ah 2 Al 1; DC refinement; Cr, Cb, Y 1-63 Ah 1 Al 0 — grayscale, 6) coded by jcphuff.c: EOB runs across blocks
 * (flushed at 0x7FFF), buffered correction bits (flushed past 937), optimal Huffman tables per scan (Y table 0, Cb / Cr
 * table 1).  The interleaved DC scans include the dummy blocks; every AC scan covers only its component's own blocks.
 * `header` is SOI .. SOF2; the device writes each scan's DHT segments (one table each, the ones the scan uses, in table-id
 * order; none for a DC refinement), its SOS and its padded, stuffed data, then EOI.  params->optimize is ignored (libjpeg
 * forces optimal tables for progressive files); only the quantisers of `tables` are read.  Workspace: 16-byte aligned,
 * >= imgxf_jpeg_workspace_bytes_prog.  Errors and limits as imgxf_jpeg_encode_ex_u8 (at most 2097143 blocks per frame);
 * sizes[f] = 0xFFFFFFFF when the file does not fit out_frame_stride (nblk * 1024 + 8192 bytes always suffice: a block
 * takes at most 4072 bits over all scans), 0xFFFFFFFE when a scan's optimal table would need a code over 32 bits. */
int imgxf_jpeg_workspace_bytes_prog(const imgxf_jpeg_enc_params* params, int n, int h, int w, size_t out_frame_stride,
                                    size_t* bytes);
int imgxf_jpeg_encode_prog_u8(const imgxf_view* src, const imgxf_jpeg_enc_params* params, const imgxf_jpeg_tables* tables,
                              const uint8_t* header, int header_bytes, uint8_t* out, size_t out_frame_stride,
                              uint32_t* sizes, void* workspace, size_t workspace_bytes, void* stream);

/* The list writer for progressive files: one call writes a LIST of frames of different sizes that share one class (ncomp,
 * sampling) as the files of imgxf_jpeg_encode_prog_u8, in a number of launches that depends on the class alone (158 for a
 * colour class, 92 for grayscale, memsets included), never on the frames.  params->optimize is ignored, as there (the block
 * states it as 1).  The block is
 *     imgxf_jpeg_list_prog_header | imgxf_jpeg_list_frame[n] | imgxf_jpeg_list_unit tables (5)
 * whose frame records and unit tables are byte for byte those imgxf_jpeg_encode_list_ex_layout_host writes for the same
 * class and sizes: every scan runs over the frame's nblk block slots (the slots past the scan's own blocks are zero-length
 * entries), so the five unit tables serve all scans.  The workspace holds the areas of the sequential list, the three
 * own-table areas (always present) and four more: per block slot, at the frame's blk_off, uint32 flags, correction-bit
 * counts and EOB-run lengths; then uint32 pos[11][n] (where each scan of each frame starts in its file, or the sizes[]
 * sentinel once a scan failed) followed by the correction-bit totals [n]. */
#define IMGXF_JPEG_LIST_PROG_AREAS 4
typedef struct imgxf_jpeg_list_prog_header {
    imgxf_jpeg_list_ex_header ex;                            /* ex.list.frames_off = sizeof(imgxf_jpeg_list_prog_header) */
    uint64_t prog_off[IMGXF_JPEG_LIST_PROG_AREAS];           /* byte offsets into the workspace, 256-byte aligned */
} imgxf_jpeg_list_prog_header;
/* HOST half, as imgxf_jpeg_encode_list_ex_layout_host.  The workspace never exceeds the sum over the frames of
 * imgxf_jpeg_workspace_bytes_prog(params, 1, h, w, capacity).  Errors as there: IMGXF_ERR_ARG for params outside the
 * classes, a capacity below 1024 + 2; IMGXF_ERR_SHAPE for h or w outside 1..32767, the block limit and more than 65535
 * frames (the table stage runs one workgroup per table and frame); IMGXF_ERR_WORKSPACE when block_cap is too small (the
 * sizes are still reported). */
int imgxf_jpeg_encode_list_prog_layout_host(const imgxf_jpeg_enc_params* params, const int32_t* sizes, const uint64_t* capacities,
                                            int n, void* block, size_t block_cap, size_t* block_bytes, size_t* workspace_bytes,
                                            size_t* out_bytes);
/* The launches, with the arguments and the contract of imgxf_jpeg_encode_list_ex_u8.  `header` is SOI .. SOF2 with any
 * size: the device writes each frame's height and width, every scan's DHT segments and SOS, its stuffed data and EOI into
 * the frame's slot.  sizes[f]: the file's length, 0xFFFFFFFF when the file does not fit out_cap (a frame that overflows in
 * some scan writes nothing past its slot in that scan or a later one; the other frames' files are unaffected), 0xFFFFFFFE
 * when a scan's optimal table would need a code over 32 bits.  Every record is checked and the block rebuilt and compared
 * before a device pointer is looked at: a block laid out for other params (or by another layout function) and a header
 * without SOF2 -> IMGXF_ERR_ARG, n > 65535 -> IMGXF_ERR_SHAPE; the other errors as imgxf_jpeg_encode_list_u8. */
int imgxf_jpeg_encode_list_prog_u8(const void* block_host, const void* block_dev, const imgxf_jpeg_enc_params* params,
                                   const imgxf_jpeg_tables* tables, const uint8_t* header, int header_bytes, uint8_t* out,
                                   size_t out_bytes, uint32_t* sizes, void* workspace, size_t workspace_bytes, void* stream);

/* JPEG compression applied in place of a file: dst = the pixels of `Image.open(f).convert("RGB")` (grayscale: the "L"
 * image) after `Image.fromarray(src).save(f, "JPEG", quality=q, subsampling=s)`, bit-identical to Pillow, for the frames
 * and layouts of imgxf_jpeg_encode_ex_u8.  Nothing is entropy-coded: one kernel runs the writer's transform stage (colour
 * conversion, downsampling, jfdctint, the quantiser) and, on the same registers, the reader's inverse (the quantiser
 * steps tables->quant — what the file's DQT would state —, jidctint islow, the range limit); for colour frames the
 * reader's colour stage (imgxf_jpeg_decode_color: fancy upsampling, jdcolor.c) then reads the component planes from the
 * workspace.  Two launches and one small host-to-device copy (the colour stage's records); grayscale: one launch, no
 * workspace (0 bytes, may be NULL).  params->optimize (0 / 1) is accepted and ignored — it does not change a pixel —, and
 * only tables->quant and ac_len are read.  src and dst: same n, h, w, c == params->ncomp, any strides, not aliased.
 * workspace: device, 16-byte aligned, >= imgxf_jpeg_roundtrip_workspace_bytes (1.5 bytes per pixel at 4:2:0, 2 at
 * 4:2:2, 3 at 4:4:4, over MCU-padded frames, + 232 bytes per frame).  Errors: a NULL view, params, tables ->
 * IMGXF_ERR_NULL; malformed views, different geometries, n > 65535 -> IMGXF_ERR_SHAPE; c != ncomp ->
 * IMGXF_ERR_UNSUPPORTED; ncomp, sampling, optimize or a quantiser out of range -> IMGXF_ERR_ARG; workspace too small or
 * misaligned -> IMGXF_ERR_WORKSPACE.  Four-component frames are out of scope.
 * The colour stage's records (n x 232 bytes) are built in pageable host memory and sent with hipMemcpyAsync on `stream`:
 * as the HIP API documents for pageable memory, the call returns once they are in the runtime's staging memory, which on
 * current runtimes means the host waits until earlier work on `stream` has drained.  A caller that must not wait uses the
 * list entry point below, whose records travel in the caller's own (pinned) block.
 * imgxf_jpeg_roundtrip_records_host (no device work) writes those n records for a colour batch whose frame f is stored at
 * byte f * out_frame_stride of the destination with rows of out_row_stride bytes: what imgxf_jpeg_layout_host reports
 * for Pillow's files of such frames, planes one frame after the other.  ncomp == 1 -> IMGXF_ERR_UNSUPPORTED (a grayscale
 * frame has no colour stage); other errors as above. */
struct imgxf_jpeg_dec_image;
int imgxf_jpeg_roundtrip_records_host(const imgxf_jpeg_enc_params* params, int n, int h, int w, int64_t out_row_stride,
                                      int64_t out_frame_stride, struct imgxf_jpeg_dec_image* images);
int imgxf_jpeg_roundtrip_workspace_bytes(const imgxf_jpeg_enc_params* params, int n, int h, int w, size_t* bytes);
int imgxf_jpeg_roundtrip_u8(const imgxf_view* src, const imgxf_view* dst, const imgxf_jpeg_enc_params* params,
                            const imgxf_jpeg_tables* tables, void* workspace, size_t workspace_bytes, void* stream);
/* The same for a LIST of RGB frames of different sizes at the default sampling (4:2:0), one quality per call, in two
 * launches whatever the list.  The HOST lays out one block
 *     imgxf_jpeg_roundtrip_list_header | imgxf_jpeg_list_frame[n] | imgxf_jpeg_dec_image[n] | imgxf_jpeg_list_unit[n_units]
 * which the caller completes (data, row_stride of every frame record) and copies to the device once.  Of a frame record
 * only data, row_stride, h .. nblk and out_off / out_cap (the frame's 16-byte aligned slot of `out` and its 3 h w bytes)
 * are used, the rest is 0; the decoder records are what imgxf_jpeg_layout_host reports for the frames' files, with the
 * frame's planes in the workspace and out_off / out_pitch = 3 w its slot.  The unit table is the writer's transform
 * stage's (16x256-pixel strips, item = strip | MCU row << 16). */
typedef struct imgxf_jpeg_roundtrip_list_header {
    int32_t  n_frames, frames_off, images_off, units_off, n_units, total_bytes;   /* byte offsets into the block; its size */
    uint64_t workspace_bytes, out_bytes;
} imgxf_jpeg_roundtrip_list_header;
/* HOST half (no device work).  sizes: int32 [n][2] = (h, w).  Writes the block (block == NULL: the sizes only) and reports
 * the block's bytes, the workspace's (the planes: 384 bytes per 16x16 MCU) and the output's.  Errors: IMGXF_ERR_NULL;
 * IMGXF_ERR_SHAPE for n < 0 or n > 65535, h or w outside 1..32767; IMGXF_ERR_ARG for a block over 2 GiB;
 * IMGXF_ERR_WORKSPACE when block_cap is too small. */
int imgxf_jpeg_roundtrip_list_layout_host(const int32_t* sizes, int n, void* block, size_t block_cap, size_t* block_bytes,
                                          size_t* workspace_bytes, size_t* out_bytes);
/* The launches: block_host is the caller's host copy of the block, block_dev the same bytes on the device (8-byte
 * aligned).  Frame f's pixels go to out + frames[f].out_off, rows of 3 w bytes.  Every record is checked on the host
 * before anything is launched, as imgxf_jpeg_encode_list_u8 checks its block: a NULL data -> IMGXF_ERR_NULL; h, w or
 * row_stride < 3 w -> IMGXF_ERR_SHAPE; a block that is not what the layout function writes for the records' (h, w) ->
 * IMGXF_ERR_ARG; workspace or `out` too small or misaligned (16 bytes) -> IMGXF_ERR_WORKSPACE. */
int imgxf_jpeg_roundtrip_list_u8(const void* block_host, const void* block_dev, const imgxf_jpeg_tables* tables, uint8_t* out,
                                 size_t out_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ---- mask stage of apply_background_change  transformation.py:340-341 -----------------*/
/* 256-bin histogram per frame of a c==1 view into hist[n][256] (uint32, device, zeroed by the call). */
int imgxf_histogram_u8(const imgxf_view* src, uint32_t* hist, void* stream);
/* mask = (src > np.percentile(src, q)) ? 255 : 0 per frame, threshold derived on the device
 * from `hist` (numpy 'linear' method).  thr_out: device double[n] (required), receives the
 * percentile of every frame. */
int imgxf_percentile_mask_u8(const imgxf_view* src, const uint32_t* hist, double q,
                             const imgxf_view* dst, double* thr_out, void* stream);
/* scipy.ndimage.binary_dilation(mask, iterations) with the 4-connected cross, border 0:
 * equals "L1 distance <= iterations" for this structuring element.  0/255 masks, c==1.
 * iterations in 1..16. */
int imgxf_dilate_cross_u8(const imgxf_view* src, const imgxf_view* dst, int iterations,
                          void* stream);

/* ---- f-4 (decode half): Image.open(path).convert("RGB")  transformation.py:83 -----------------------
 * Baseline / extended-sequential Huffman JPEG, 8 bit, 1 or 3 components (Y or YCbCr; 4:4:4, 4:2:2 h2v1, 4:2:0 h2v2),
 * decoded the way Pillow's libjpeg-turbo does with its defaults: jpeg_idct_islow, fancy (triangle) upsampling, the
 * 16-bit fixed-point YCbCr -> RGB tables, grayscale replicated — bit-identical pixels.  The HOST parses the markers,
 * removes the byte stuffing, splits the scan at RSTn markers and derives the lookup tables (imagetransformations_amd/
 * jpeg.py); the device does the entropy decoding (one thread per restart segment — a file without restart markers is one
 * segment: Huffman decoding is the serial direction), dequantisation + IDCT, upsampling and colour conversion.
 * All arrays are DEVICE pointers; offsets are in elements of the array they index. */
typedef struct imgxf_jpeg_dec_comp {
    int32_t h, v;               /* sampling factors (1 or 2) */
    int32_t dc_tab, ac_tab;     /* indices into luts[] (imgxf_jpeg_dec_lut) */
    int32_t quant;              /* index into quants[] (64 uint16 each, natural order) */
    int32_t blocks_x, blocks_y; /* allocated blocks: mcux * h, mcuy * v */
    int32_t dw, dh;             /* downsampled_width / height: ceil(width * h / hmax), ceil(height * v / vmax) */
    int64_t coef_off;           /* first int16 coefficient of the component in coefs[] ([blocks_y][blocks_x][64], ZIGZAG order: the stream's) */
    int64_t plane_off;          /* first byte of the component's sample plane in planes[] (pitch = 8 * blocks_x) */
} imgxf_jpeg_dec_comp;
typedef struct imgxf_jpeg_dec_image {
    int32_t width, height, ncomp, hmax, vmax, mcux, mcuy;
    int32_t restart_interval;   /* MCUs per segment (the whole scan when the file has no DRI) */
    int32_t seg_first, seg_count; /* this image's entries of seg_off[] (byte offset of each segment in scan[]) and seg_len[] */
    int32_t pad_;
    int64_t out_off;            /* first byte of the image's RGB pixels in out[] (row pitch = out_pitch bytes) */
    int64_t out_pitch;
    imgxf_jpeg_dec_comp comp[3];
} imgxf_jpeg_dec_image;
typedef struct imgxf_jpeg_dec_lut {
    uint16_t look[256];         /* 8-bit lookahead: (code length << 8) | symbol, 0 = the code is longer than 8 bits */
    int32_t  maxcode[18];       /* jdhuff.c: largest code of each length (index 1..16), -1 if none; [17] = sentinel */
    int32_t  valoff[17];        /* huffval index of the first code of each length minus that code */
    uint8_t  huffval[256];
} imgxf_jpeg_dec_lut;
/* Entropy decoding of n images: coefs[] must be ZERO on entry (only non-zero coefficients are written).  status[i]
 * (device int32, may be NULL) receives 0, or 1 when image i's stream held an impossible code / ran out of data. */
int imgxf_jpeg_decode_huffman(const uint8_t* scan, const int64_t* seg_off, const int32_t* seg_len,
                              const imgxf_jpeg_dec_image* images, int n, const imgxf_jpeg_dec_lut* luts,
                              int16_t* coefs, int32_t* status, void* stream);
/* HOST helper of the reader (no device work): walks the entropy-coded bytes of one file's scan from data[start], removes
 * the byte stuffing (FF 00 -> FF), splits at RSTn and stops at the first other marker (or at n; *ecs_end = that position).
 * At most max_segs segments are kept (the scan's ceil(MCUs / restart interval); later ones are skipped).  Segment k is
 * written to scan[] at seg_off[k] (16-byte aligned, taken from *scan_pos, which is advanced) with seg_len[k] bytes followed
 * by 16 .. 31 zero bytes.  IMGXF_ERR_WORKSPACE if scan_cap is too small.  Replaces the per-byte Python walk of
 * jpeg_decode._segments for the batched reader (load_data's Image.open, /root/reference/transformation.py:73-89). */
int imgxf_jpeg_unstuff_host(const uint8_t* data, size_t n, size_t start, uint8_t* scan, size_t scan_cap, size_t* scan_pos,
                            int64_t* seg_off, int32_t* seg_len, int max_segs, int* nsegs, size_t* ecs_end);
/* NumPy's legacy generator on the device (np.random.normal of apply_gaussian_noise, /root/reference/transformation.py:273-275):
 * the raw MT19937 state sequence — out[0 .. 623] = key (device pointer, the generator's current 624 state words), block b =
 * the state after b regenerations (mt19937_gen), (nblocks + 1) * 624 words in all; nblocks = 0 writes the key only.  One
 * workgroup: the recurrence is sequential in the block index.  This is imgxf_mt19937_stretches' kernel launched with one
 * stretch of nblocks + 1 blocks from `key`, so both entry points run the same block loop.  Tempering, legacy_double and the
 * polar method follow in imagetransformations_amd/numpy_stream.py. */
int imgxf_mt19937_blocks(const uint32_t* key, uint32_t* out, int64_t nblocks, void* stream);

/* The same sequence in parallel.  imgxf_mt19937_jump: out_keys[w * 624 ..] = the generator's canonical state (w + 1) * J words
 * after base_key[0 .. 623], for w = 0 .. n_out - 1, all in parallel; J = 624 * 2^k words is the stride whose jump polynomials
 * `coefs` holds ([n_out][2496] bytes: 19937 coefficients each, little-endian bits; imagetransformations_amd/mt19937_jump.npz,
 * written and checked by tools/make_mt_jump.py).  Word 0 of a jumped state is state only in its top bit.
 * imgxf_mt19937_stretches: workgroup m writes blocks m * blocks_per_stretch .. of the state sequence from keys[m]; total_blocks
 * in all.  Together they produce exactly what imgxf_mt19937_blocks produces. */
int imgxf_mt19937_jump(const uint32_t* base_key, uint32_t* out_keys, int n_out, const uint8_t* coefs, void* stream);
int imgxf_mt19937_stretches(const uint32_t* keys, uint32_t* out, int n_stretches, int64_t blocks_per_stretch, int64_t total_blocks,
                            void* stream);

/* NumPy's legacy_gauss over the word stream of imgxf_mt19937_blocks / _stretches (numpy/random/src/legacy/legacy-distributions.c
 * restated; imagetransformations_amd/numpy_stream.py): group g = four consecutive words -> (x1, x2, r2), accepted iff 0 < r2 < 1.
 * imgxf_np_accept writes the acceptance flags; with their inclusive prefix sum `rank`, imgxf_np_normals_f32 writes the float32
 * results of consecutive np.random.normal(0, scale, count) calls: accepted group k <= groups yields normals 2 (k - 1), 2 (k - 1) + 1
 * (f x2 then f x1) of n2; out[e + lead] = float(0.0 + scale * f x) with the scale of the request whose range (reqs: {int64 begin,
 * double scale} sorted by begin, positions counted with `lead` = 1 if a cached normal precedes) holds it.  Samples within `margin`
 * (relative) of a float32 rounding boundary are listed in risky[] (info[1] = how many; the host recomputes them with its libm);
 * info[0] = the index of the groups-th accepted group, xr[0 .. 1] = its (x1, r2), xr[2 + 2 s ..] = (x, r2) of risky sample s
 * (xr holds 2 + 2 risky_cap doubles). */
int imgxf_np_accept(const uint32_t* words, int64_t ngroups, uint8_t* acc, void* stream);
int imgxf_np_normals_f32(const uint32_t* words, int64_t ngroups, const int64_t* rank, int64_t groups, int64_t n2, int lead,
                         const void* reqs, int nreq, double margin, float* out, int64_t* info, int64_t* risky, int64_t risky_cap,
                         double* xr, void* stream);

/* A list of MIXED legacy calls in call order over the same word stream — np.random.normal(0, scale, count), np.random.random(count)
 * and scalar np.random.randint(low, high) — in two launches (imagetransformations_amd/numpy_stream.py `mixed` states the rules and
 * builds the tables).  words: the raw stream, nwords of it; pos: the generator's position.  reqs: nreq records of 64 bytes
 * {int32 kind (0 normal, 1 random, 2 randint), int32 lead (normal: 0, or the first sample is the cached normal — 1: the one the call
 * starts with, value gauss0; 2: one an earlier request left), int64 count, double scale, int64 out_off (bytes into out), int64 tab_off,
 * int64 max_chunks, uint32 rng, uint32 mask, int64 blk0}.  chunk: the groups per chunk the tables were built for (4096; anything else
 * is IMGXF_ERR_ARG).
 * imgxf_np_mixed_walk, ONE workgroup, serial over the requests and parallel inside each: writes walk[i] = {int64 start position, int64
 * chunks used, double x1, r2 of a lead of kind 2}, table[tab_off + c] = accepted groups of the request before its chunk c, ints[i] =
 * v <= rng of a randint (the host adds low), info[0] = error (1: the stream ended, 2: a request needed more than max_chunks; the walk
 * stops there and never reads past nwords), info[1] = final position, info[2 .. 3] = bits of (x1, r2) of the cached normal the list
 * leaves.  info holds 8 words, zeroed by the caller.
 * imgxf_np_mixed_fill, one workgroup per (request, chunk) — block_req[b] = request of workgroup b, nblocks of them, blk0 = the
 * request's first: writes the doubles of random requests and float(0.0 + scale * f x) (f64: the double) of normal requests into out.
 * Samples within `margin` of a float32 rounding boundary (relative; f64: of an integer, absolute) are appended to risky[] as {request,
 * index in its results, bits of x, bits of r2} (risky_cap entries of 4 words; info[4] counts all of them) for the host's libm.
 * Nothing is written if the walk reported an error. */
int imgxf_np_mixed_walk(const uint32_t* words, int64_t nwords, int64_t pos, const void* reqs, int nreq, int chunk, void* walk,
                        int64_t* table, int64_t* ints, int64_t* info, void* stream);
int imgxf_np_mixed_fill(const uint32_t* words, int64_t nwords, const void* reqs, const int32_t* block_req, int64_t nblocks, int chunk,
                        const void* walk, const int64_t* table, double gauss0, int f64, double margin, void* out, int64_t* info,
                        int64_t* risky, int64_t risky_cap, void* stream);

/* Why a file is outside the reader's class, or damaged (status[] of imgxf_jpeg_layout_host; 0 = accepted). */
enum { IMGXF_JPEG_E_NOT_JPEG = 1,    /* no SOI */
       IMGXF_JPEG_E_MARKERS = 2,     /* damaged marker structure (also: SOS before SOF) */
       IMGXF_JPEG_E_PRECISION = 3,   /* samples are not 8 bits */
       IMGXF_JPEG_E_PROCESS = 4,     /* progressive, lossless or arithmetic coding */
       IMGXF_JPEG_E_COMPONENTS = 5,  /* neither 1 nor 3 components, or a non-interleaved scan */
       IMGXF_JPEG_E_SCAN_ORDER = 6,  /* the scan names an unknown component or not in frame order */
       IMGXF_JPEG_E_SAMPLING = 7,    /* sampling factors outside 1..2 */
       IMGXF_JPEG_E_CHROMA = 8,      /* chroma sampling other than 4:4:4, 4:2:2 (h2v1), 4:2:0 */
       IMGXF_JPEG_E_NO_QUANT = 9,    /* a component's quantisation table is missing */
       IMGXF_JPEG_E_NO_HUFF = 10,    /* a component's Huffman table is missing */
       IMGXF_JPEG_E_TRUNCATED = 11   /* the scan ends before its last restart segment */ };
/* HOST half of the reader for a batch of n files (no device work; csrc/jpeg_layout.hip): marker segments up to the scan
 * (jdmarker.c), image / component descriptors, quantisation tables in natural order, derived Huffman tables
 * (jpeg_make_d_derived_tbl; equal tables are shared), and the entropy-coded bytes laid out by imgxf_jpeg_unstuff_host.
 * Pass 1, scan == NULL: only the counts — *n_segs, *n_quants, *n_luts and *scan_bytes are (bounds on) what pass 2 needs.
 * Pass 2: images[n], luts[*n_luts], quants[*n_quants][64], scan[*scan_bytes], seg_off / seg_len[*n_segs] are filled,
 * *coef_total / *plane_total are the sizes of coefs[] (int16) and planes[] (bytes); out_off / out_pitch of the images are
 * left to the caller.  status[i] is 0 or the IMGXF_JPEG_E_* code of file i; the call returns IMGXF_OK unless a capacity
 * is too small (IMGXF_ERR_WORKSPACE).  Replaces Image.open's header parsing, /root/reference/transformation.py:83. */
int imgxf_jpeg_layout_host(const uint8_t* const* files, const size_t* sizes, int n, imgxf_jpeg_dec_image* images,
                           imgxf_jpeg_dec_lut* luts, int lut_cap, int* n_luts, uint16_t* quants, int quant_cap, int* n_quants,
                           uint8_t* scan, size_t scan_cap, size_t* scan_bytes, int64_t* seg_off, int32_t* seg_len, int seg_cap,
                           int* n_segs, int64_t* coef_total, int64_t* plane_total, int32_t* status);
/* Dequantisation + jpeg_idct_islow of every block of n images into their sample planes. */
int imgxf_jpeg_decode_idct(const int16_t* coefs, const imgxf_jpeg_dec_image* images, const imgxf_jpeg_dec_image* images_host,
                           int n, const uint16_t* quants, uint8_t* planes, void* stream);
/* Fancy upsampling + YCbCr -> RGB (or gray -> RGB) of n images into out[] (HWC uint8 RGB at out_off / out_pitch). */
int imgxf_jpeg_decode_color(const uint8_t* planes, const imgxf_jpeg_dec_image* images, const imgxf_jpeg_dec_image* images_host,
                            int n, uint8_t* out, void* stream);

/* ---- the same load step for PROGRESSIVE files (SOF2, Huffman, 8 bit, 1 or 3 components, the samplings above) ---------
 * Only the way the quantised coefficients reach coefs[] differs from a baseline file (libjpeg-turbo jdcoefct.c
 * decompress_data over the whole-image buffer): imgxf_jpeg_decode_idct and imgxf_jpeg_decode_color are reused as they
 * are.  Refusal codes after IMGXF_JPEG_E_TRUNCATED (status[] of imgxf_jpeg_layout_progressive_host): */
enum { IMGXF_JPEG_E_SCAN_SCRIPT = 12, /* a progression jdphuff.c start_pass_phuff_decoder rejects or warns about (bad Ss / Se /
                                         Ah / Al, an AC scan of several components or before the component's DC, Ah not the
                                         previous Al) */
       IMGXF_JPEG_E_SMOOTHING = 13,   /* jdcoefct.c smoothing_ok would hold: after the last scan a component's coefficient
                                         1..9 is not fully refined, so libjpeg would smooth blocks (not restated) */
       IMGXF_JPEG_E_COLORSPACE = 14   /* a 3-component file jdapimin.c default_decompress_parms does not read as YCbCr (no
                                         JFIF marker, and Adobe transform 0 (or unknown), or component ids 'R','G','B') */ };
/* One scan of a progressive file (jdphuff.c: Ss..Se is the spectral band in zigzag order, Ah / Al the successive
 * approximation bits; a DC scan (Ss = 0) may hold several components and is then interleaved in the MCU order of the frame,
 * dummy blocks included; every other scan holds one component and visits its ceil(dw / 8) x ceil(dh / 8) blocks in raster
 * order).  Rows of one image are contiguous and in file order. */
typedef struct imgxf_jpeg_dec_scan {
    int32_t image;              /* index into images[] */
    int32_t ncomp;              /* components in the scan */
    int32_t comp[3];            /* their indices in the image's comp[] (increasing) */
    int32_t ss, se, ah, al;
    int32_t dc_tab[3];          /* luts[] of each scan component's DC table (DC first scans), else -1 */
    int32_t ac_tab;             /* luts[] of the AC table (AC scans), else -1 */
    int32_t restart_interval;   /* MCUs (blocks, in a one-component scan) per segment: the whole scan without DRI */
    int32_t seg_first, seg_count; /* this scan's entries of seg_off[] / seg_len[] */
    int32_t level;              /* 0 when no earlier scan of the image shares a component and overlaps its band, else
                                   1 + the largest level of those that do: scans of one level can run in any order */
} imgxf_jpeg_dec_scan;
/* HOST half for progressive files, beside imgxf_jpeg_layout_host and with its two-call protocol: pass 1 (scan == NULL)
 * gives bounds on *n_scans, *n_segs, *n_quants, *n_luts, *scan_bytes; pass 2 fills images[n] (the descriptor of
 * imgxf_jpeg_layout_host: MCU-padded blocks_x / blocks_y, coef_off, plane_off; restart_interval / seg_first / seg_count
 * are 0, the scans carry them), scans[*n_scans] (the rows of file i contiguous), luts, quants (latched per component at
 * its first scan: jdinput.c latch_quant_tables) and the unstuffed, RSTn-split, 16-byte aligned segments of every scan
 * (imgxf_jpeg_unstuff_host).  Every marker from SOI to EOI is walked (jdmarker.c); a file that ends before EOI, or whose
 * scan ends before its last restart segment, is IMGXF_JPEG_E_TRUNCATED.  Baseline files are IMGXF_JPEG_E_PROCESS here. */
int imgxf_jpeg_layout_progressive_host(const uint8_t* const* files, const size_t* sizes, int n, imgxf_jpeg_dec_image* images,
                                       imgxf_jpeg_dec_scan* scans, int scans_cap, int* n_scans,
                                       imgxf_jpeg_dec_lut* luts, int lut_cap, int* n_luts, uint16_t* quants, int quant_cap,
                                       int* n_quants, uint8_t* scan, size_t scan_cap, size_t* scan_bytes, int64_t* seg_off,
                                       int32_t* seg_len, int seg_cap, int* n_segs, int64_t* coef_total, int64_t* plane_total,
                                       int32_t* status);
/* Progressive entropy decoding (jdphuff.c decode_mcu_DC_first / _AC_first / _DC_refine / _AC_refine, EOBRUN, the DC
 * predictors and EOBRUN reset at every RSTn) of n images into coefs[] (ZERO on entry; the zigzag layout
 * imgxf_jpeg_decode_idct reads).  One workgroup per image; its lanes take the (scan, restart segment) pairs of one
 * dependency level at a time.  status[i] (device, may be NULL) receives 1 when image i's data held an impossible code or
 * ran out; its loops then end — damaged data never writes outside the image's blocks.  All pointers but `images_host`
 * are device pointers; scans_host is the host copy of scans[] (its rows are checked before the launch). */
int imgxf_jpeg_decode_progressive(const uint8_t* scan, const int64_t* seg_off, const int32_t* seg_len,
                                  const imgxf_jpeg_dec_scan* scans, const imgxf_jpeg_dec_scan* scans_host, int n_scans,
                                  const imgxf_jpeg_dec_image* images, int n, const imgxf_jpeg_dec_lut* luts, int16_t* coefs,
                                  int32_t* status, void* stream);
/* imgxf_jpeg_layout_host and the Python parse refuse a 3-component baseline file that default_decompress_parms does not read
 * as YCbCr with IMGXF_JPEG_E_COLORSPACE too: the reader above converts every 3-component file as YCbCr. */

/* ---- the same load step for EXTENDED sequential files: 3 or 4 components, any sampling libjpeg accepts ----------------
 * SOF0 / SOF1 Huffman, 8 bit, all components in one interleaved scan; colour space as jdapimin.c default_decompress_parms
 * chooses it (3 components: JFIF -> YCbCr, else Adobe transform 0 -> RGB / other -> YCbCr, else ids 'R','G','B' -> RGB,
 * else YCbCr; 4 components: Adobe transform 0 -> CMYK / other -> YCCK, no Adobe marker -> CMYK); each h, v in 1..4 with
 * hmax / h and vmax / v integral and at most 10 blocks per MCU (D_MAX_BLOCKS_IN_MCU).  Output: the RGB pixels of
 * Image.open(f).convert("RGB") — for 4 components libjpeg's ycck_cmyk_convert (YCCK), Pillow's "CMYK;I" rawmode (every
 * sample inverted) and Pillow's cmyk2rgb.  Refusal codes after IMGXF_JPEG_E_COLORSPACE (status[] of
 * imgxf_jpeg_layout_extended_host, which also uses E_COMPONENTS for other than 3 or 4 components and E_SAMPLING for
 * factors outside 1..4): */
enum { IMGXF_JPEG_E_FRACTIONAL = 15,  /* hmax / h or vmax / v not integral (jdsample.c JERR_FRACT_SAMPLE_NOTIMPL) */
       IMGXF_JPEG_E_MCU_SIZE = 16     /* more than 10 blocks per MCU (jdinput.c JERR_BAD_MCU_SIZE) */ };
enum { IMGXF_JPEG_CS_YCBCR = 0, IMGXF_JPEG_CS_RGB = 1, IMGXF_JPEG_CS_CMYK = 2, IMGXF_JPEG_CS_YCCK = 3 };
typedef struct imgxf_jpeg_dec_image_ext {
    int32_t width, height, ncomp, hmax, vmax, mcux, mcuy;   /* as imgxf_jpeg_dec_image; ncomp 3 or 4 */
    int32_t restart_interval, seg_first, seg_count;
    int32_t color;              /* IMGXF_JPEG_CS_* */
    int32_t blocks_in_mcu;      /* 1 .. 10 */
    uint8_t mcu_comp[10];       /* block b of an MCU: component mcu_comp[b], block (mcu_bx[b], mcu_by[b]) of its h x v */
    uint8_t mcu_bx[10], mcu_by[10];
    uint8_t pad_[2];
    int64_t out_off, out_pitch;
    imgxf_jpeg_dec_comp comp[4]; /* h, v in 1..4; the rest as in imgxf_jpeg_dec_image */
} imgxf_jpeg_dec_image_ext;
/* HOST half for extended files: imgxf_jpeg_layout_host's two-call protocol and arrays, with imgxf_jpeg_dec_image_ext
 * descriptors (pass 1: *n_luts is a bound of 8 per file). */
int imgxf_jpeg_layout_extended_host(const uint8_t* const* files, const size_t* sizes, int n, imgxf_jpeg_dec_image_ext* images,
                                    imgxf_jpeg_dec_lut* luts, int lut_cap, int* n_luts, uint16_t* quants, int quant_cap, int* n_quants,
                                    uint8_t* scan, size_t scan_cap, size_t* scan_bytes, int64_t* seg_off, int32_t* seg_len, int seg_cap,
                                    int* n_segs, int64_t* coef_total, int64_t* plane_total, int32_t* status);
/* The three device stages of imgxf_jpeg_decode_huffman / _idct / _color over extended descriptors: entropy decoding (a lane
 * per restart segment, or the in-segment parallel decoder for long segments), dequantisation + jpeg_idct_islow, and
 * upsampling (jdsample.c: fullsize, h2v1 / h2v2 fancy when downsampled_width > 2, h1v2 fancy, int_upsample otherwise)
 * + colour conversion into the RGB frames at out_off / out_pitch.  images_host: the host copy, checked before a launch. */
int imgxf_jpeg_decode_huffman_ext(const uint8_t* scan, const int64_t* seg_off, const int32_t* seg_len,
                                  const imgxf_jpeg_dec_image_ext* images, const imgxf_jpeg_dec_image_ext* images_host, int n,
                                  const imgxf_jpeg_dec_lut* luts, int16_t* coefs, int32_t* status, void* stream);
int imgxf_jpeg_decode_idct_ext(const int16_t* coefs, const imgxf_jpeg_dec_image_ext* images, const imgxf_jpeg_dec_image_ext* images_host,
                               int n, const uint16_t* quants, uint8_t* planes, void* stream);
int imgxf_jpeg_decode_color_ext(const uint8_t* planes, const imgxf_jpeg_dec_image_ext* images, const imgxf_jpeg_dec_image_ext* images_host,
                                int n, uint8_t* out, void* stream);

/* ---- the evaluation preprocessing of the reference's ImageNet scripts on a LIST of frames of different sizes ----------
 * transforms.Compose([Resize(r), CenterCrop(crop), ToTensor(), Normalize(mean, std)]) on each RGB frame of a list, as
 * Pillow / torchvision compute it on PIL images (BILINEAR Image.resize: horizontal pass, uint8 intermediate, vertical
 * pass, 22-bit coefficients; only the crop window is filtered), all frames in ONE launch.  The HOST lays out one block
 *     imgxf_preprocess_header | imgxf_preprocess_frame[n] | imgxf_preprocess_unit[n_units] | int32 tables
 * which the caller copies to the device once; offsets of tables are int32 indices into the block. */
typedef struct imgxf_preprocess_header {
    int32_t n_frames, n_units, crop;
    int32_t lds_bytes;          /* the largest unit's LDS need = the launch's dynamic LDS size */
    int32_t frames_off, units_off, tables_off, total_bytes;   /* byte offsets of the sections, size of the block */
} imgxf_preprocess_header;
typedef struct imgxf_preprocess_frame {
    uint64_t data;              /* DEVICE address of pixel (0, 0); filled by the caller, as is row_stride (bytes, >= 3 w) */
    int64_t  row_stride;
    int32_t  h, w;
    int32_t  ksx, ksy;          /* taps per output column / row (row length of the coefficient tables) */
    int32_t  bounds_x, coeffs_x, bounds_y, coeffs_y;   /* [crop][2] (first source index, count), [crop][ks]; frames of
                                   equal geometry share them */
    int32_t  row0, nrows, col0, ncols;   /* the source rows / columns the crop window touches */
    int32_t  unit_rows;         /* output rows per work unit; 0: the frame exceeds the LDS budget and has no units */
    int32_t  pad_;
} imgxf_preprocess_frame;
typedef struct imgxf_preprocess_unit {
    int32_t frame, y0, ny;      /* one workgroup: output rows [y0, y0 + ny) of the crop window of frame `frame` */
    int32_t lds_bytes;          /* touched source rows x 12 ceil(crop / 4) (rounded up to 16) + 4 staged source-row spans */
} imgxf_preprocess_unit;
/* HOST half (no device work).  geometry: int32 [n][6] = (h, w, nh, nw, left, top) per frame — source size, size after
 * Resize, crop offsets (the caller states torchvision's rule).  The tables are precompute_coeffs' for (w -> nw) and
 * (h -> nh), rows [left, left + crop) / [top, top + crop).  A unit takes up to 16 output rows, fewer where their touched
 * source rows would not fit half of lds_budget bytes (three quarters, then the whole of it, where not even one row fits
 * the smaller step; lds_budget is capped at 64 KiB, so that two workgroups fit a CU); a frame of which not even one row fits gets unit_rows = 0.  *block_bytes receives the block's size; block == NULL: only that.
 * Errors: IMGXF_ERR_NULL; IMGXF_ERR_ARG for n < 0, crop < 1, lds_budget < 1, a size < 1, h or w > 32767, nh or nw > 2^24, a window outside the
 * resized image; IMGXF_ERR_WORKSPACE when block_cap is too small. */
int imgxf_preprocess_list_layout_host(const int32_t* geometry, int n, int crop, int lds_budget, void* block,
                                      size_t block_cap, size_t* block_bytes);
/* The same with Resize's filter stated: any IMGXF_RESAMPLE_* (the tables are host-built, so all five are taken; another
 * value: IMGXF_ERR_ARG).  ksx, ksy, the LDS bounds and unit_rows follow the filter's taps, 2 ceil(support max(in / out, 1)) + 1
 * with support 0.5 (BOX), 1 (BILINEAR, HAMMING), 2 (BICUBIC), 3 (LANCZOS): with equal scales on both axes one output row
 * fits 64 KiB at crop 224 up to a 19-fold (BOX), 16-fold (BILINEAR, HAMMING), 11-fold (BICUBIC), 9-fold (LANCZOS)
 * reduction.  imgxf_preprocess_list_layout_host is this call with IMGXF_RESAMPLE_BILINEAR; imgxf_preprocess_list_f32 reads
 * the tables from the block and serves every filter.  Coefficients are signed 22-bit fixed point with |k| < 2, so a
 * product with a byte fits the kernel's 24-bit multiply and a row's sum its int32 accumulator. */
int imgxf_preprocess_list_layout_filter_host(const int32_t* geometry, int n, int crop, int filter, int lds_budget, void* block,
                                             size_t block_cap, size_t* block_bytes);
/* The launch: block_host is the caller's host copy of the block (its records are checked before the launch), block_dev
 * the same bytes on the device (8-byte aligned).  out: float32 [n][3][crop][crop], contiguous; slots of frames without
 * units are not written.  mean / std: HOST float[3], both or neither. */
int imgxf_preprocess_list_f32(const void* block_host, const void* block_dev, float* out, const float* mean,
                              const float* std, void* stream);

/* ---- per-entry resized crops (RandomResizedCrop, TTA crops) of a LIST of frames of different sizes -------------------
 * Entry k is torchvision's F.resized_crop(img, top, left, height, width, (sh, sw), BILINEAR), then F.hflip where its flip
 * flag is set, on the PIL image — Image.crop(box).resize((sw, sh), BILINEAR): coefficient windows clamped to the box —
 * and then either ToTensor() + Normalize(mean, std) (float32 planar) or the uint8 bytes themselves, all entries in ONE
 * launch.  Image.resize filters rows before columns where the box is more than 100 times as tall as wide and loses rows;
 * so does the kernel (imgxf_resized_crop_entry.tall).  Several entries may read one frame.  The HOST lays out one block
 *     imgxf_resized_crop_header | imgxf_resized_crop_entry[n] | imgxf_resized_crop_unit[n_units]
 * which the caller copies to the device once.  It holds NO coefficient table: every workgroup computes the
 * precompute_coeffs + normalize_coeffs_8bpc tables of its own unit in fp64 into LDS. */
typedef struct imgxf_resized_crop_header {
    int32_t n_entries, n_units, sh, sw;
    int32_t lds_bytes;          /* the largest unit's LDS bound = the launch's dynamic LDS size */
    int32_t entries_off, units_off, total_bytes;   /* byte offsets of the sections, size of the block */
} imgxf_resized_crop_header;
typedef struct imgxf_resized_crop_entry {
    uint64_t data;              /* DEVICE address of pixel (0, 0) of the FRAME; filled by the caller, as is row_stride
                                   (bytes, >= 3 w) */
    int64_t  row_stride;
    int32_t  h, w;              /* the frame */
    int32_t  top, left, bh, bw; /* the box, inside the frame */
    int32_t  flip;              /* 1: output column x is stored at sw - 1 - x */
    int32_t  ksx, ksy;          /* taps per output column / row: 2 ceil(support max(bw / sw, 1)) + 1, likewise for rows
                                   (support 1: BILINEAR; the *_filter calls below: 0.5 BOX, 2 BICUBIC) */
    int32_t  unit_rows;         /* output rows per work unit; 0: the entry exceeds the LDS budget and has no units */
    int32_t  lds_bytes;         /* LDS bound of a unit of unit_rows rows */
    int32_t  tall;              /* 1 where bh > 100 bw and sh < bh: Image.resize then runs its vertical pass first */
} imgxf_resized_crop_entry;
typedef struct imgxf_resized_crop_unit {
    int32_t entry, y0, ny;      /* one workgroup: output rows [y0, y0 + ny) of entry `entry` */
    int32_t lds_bytes;          /* tables 4 (sw (2 + ksx) + ny (2 + ksy)) (rounded up to 16) + R x 12 ceil(sw / 4) (rounded up
                                   to 16) + 4 staged spans of C source columns, (3 C + 6) & ~3 bytes each, with the bounds
                                   R = min(bh, ceil((ny - 1) bh / sh) + ksy), C = min(bw, ceil((sw - 1) bw / sw) + ksx);
                                   a tall entry: R x 12 ceil(bw / 4) in place of the second term, plus ny x 12 ceil(bw / 4)
                                   and ny x 12 ceil(sw / 4), each rounded up to 16 */
} imgxf_resized_crop_unit;
/* HOST half (no device work).  geometry: int32 [n][7] = (h, w, top, left, bh, bw, flip) per entry.  A unit takes up to 16
 * output rows, fewer where its LDS bound would not fit half of lds_budget bytes (three quarters, then the whole of it,
 * where not even one row fits the smaller step; lds_budget is capped at 64 KiB); an entry of which not even one row fits
 * gets unit_rows = 0.  *block_bytes receives the block's size; block == NULL: only that.
 * Errors: IMGXF_ERR_NULL; IMGXF_ERR_ARG for n < 0, sh or sw outside 1..32767, lds_budget < 1, h or w outside 1..32767, a
 * box that is empty or not inside its frame, a flip other than 0 / 1; IMGXF_ERR_WORKSPACE when block_cap is too small. */
int imgxf_resized_crop_list_layout_host(const int32_t* geometry, int n, int sh, int sw, int lds_budget, void* block,
                                        size_t block_cap, size_t* block_bytes);
/* The launch: block_host is the caller's host copy of the block, block_bytes its size (every record is checked against its
 * frame, the block and the launch's LDS before the launch; nothing past block_bytes is read), block_dev the same bytes on
 * the device (8-byte aligned).  out_u8 == 0: out is float32 [n][3][sh][sw]; mean / std HOST float[3], both or neither.
 * out_u8 == 1: out is uint8 [n][sh][sw][3]; mean / std must be NULL.  Slots of entries without units are not written. */
int imgxf_resized_crop_list(const void* block_host, size_t block_bytes, const void* block_dev, void* out, int out_u8,
                            const float* mean, const float* std, void* stream);
/* The two calls with the filter of Image.resize stated (the block's layout is the same: its records have no field for the
 * filter, so the caller passes the same value to both).  The layout takes any IMGXF_RESAMPLE_* (another value:
 * IMGXF_ERR_ARG); ksx, ksy, the LDS bounds and unit_rows follow 2 ceil(support max(box / out, 1)) + 1 taps, `tall` does not
 * depend on the filter.  The launch builds the tables of the polynomial filters — BILINEAR, BICUBIC, BOX: IEEE operations
 * alone, so the device's fp64 gives precompute_coeffs' doubles — and refuses HAMMING and LANCZOS (sin, cos) with
 * IMGXF_ERR_UNSUPPORTED; it checks every record's ksx / ksy against the filter it is given (IMGXF_ERR_ARG).  With equal
 * scales on both axes one output row fits 64 KiB at sw = 224 up to a 14-fold (BOX), 10-fold (BILINEAR), 6-fold (BICUBIC)
 * reduction.  The two calls above are these with IMGXF_RESAMPLE_BILINEAR. */
int imgxf_resized_crop_list_layout_filter_host(const int32_t* geometry, int n, int sh, int sw, int filter, int lds_budget,
                                               void* block, size_t block_cap, size_t* block_bytes);
int imgxf_resized_crop_list_filter(const void* block_host, size_t block_bytes, const void* block_dev, void* out, int out_u8,
                                   int filter, const float* mean, const float* std, void* stream);

/* ---- Image.resize of a LIST of frames of different sizes, every entry to a size of its own ----------------------------
 * Entry k is Image.fromarray(frame)[.crop(box)].resize((ow, oh), filter) for any of the five convolution filters, uint8 in
 * and uint8 out, all entries in ONE launch; the box is the image (coefficient windows clamped to it).  Several entries
 * may read one frame.  The HOST lays out one block
 *     imgxf_resize_list_header | imgxf_resize_list_entry[n] | imgxf_resize_list_unit[n_units] | int32 tables
 * which the caller copies to the device once.  The tables are precompute_coeffs' for (bw -> ow) and (bh -> oh), appended
 * once per distinct (in, out) axis of the call's filter and shared by every entry with that axis; offsets of tables are
 * int32 indices into the block.  The outputs are [oh][ow][3] uint8, contiguous, each at its entry's out_off (a multiple of
 * 16) in ONE output buffer of out_bytes bytes.
 *
 * A work unit is a band of rows AND a chunk of columns: output rows [y0, y0 + ny) x columns [x0, x0 + nx) of one entry.
 * Its workgroup keeps in LDS the horizontally filtered source rows the band touches, nx pixels wide (R x 12 ceil(nx / 4)
 * bytes, rounded up to 16), and four staged spans of the C source columns the chunk's own windows touch ((3 C + 6) & ~3
 * bytes each).  THE RULE (the one statement; `budget` = lds_budget capped at 64 KiB):
 *   chunk:     for parts = 1, 2, 4, ...: nx = min(ow, ceil(ow / parts) rounded up to 4); the entry takes the first nx for
 *              which rows(nx) > 0; where nx has come down to 4 (or ow < 4) and rows(nx) == 0 the entry is refused.  So an
 *              entry keeps the full width whenever one band fits, and only wide outputs and deep reductions are cut.
 *   rows(nx):  the most ny in 1 .. min(oh, 16) with lds(ny, nx) <= budget / 2; where none, with <= budget / 4 * 3; where
 *              none, with <= budget; else 0 (the three steps of the older list kernels: five, three, two workgroups per CU)
 *   lds(ny, nx) = r16(R x 12 ceil(nx / 4)) + 4 ((3 C + 6) & ~3),  R = min(bh, ceil((ny - 1) bh / oh) + ksy),
 *                                                                 C = min(bw, ceil((nx - 1) bw / ow) + ksx)
 *   with ks = 2 ceil(support max(in / out, 1)) + 1 taps per axis.  Chunks are x0 = 0, nx, 2 nx, ...: x0 is a multiple of 4
 *   and so is every chunk's width but the last one's.  A unit's own lds_bytes is the same expression with the R and C its
 *   tables really touch (never more than the bounds).
 * An entry is also refused (unit_rows == 0) where Image.resize filters rows before columns: a box more than 100 times as
 * tall as wide that loses rows (bh > 100 bw and oh < bh).  The caller serves refused entries by another route. */
typedef struct imgxf_resize_list_header {
    int32_t n_entries, n_units;
    int32_t lds_bytes;          /* the largest unit's LDS need = the launch's dynamic LDS size */
    int32_t pad_;
    int32_t entries_off, units_off, tables_off, total_bytes;   /* byte offsets of the sections, size of the block */
    int64_t out_bytes;          /* size of the output buffer: the end of the last entry's slot (refused entries have slots
                                   too, which the launch does not write) */
} imgxf_resize_list_header;
typedef struct imgxf_resize_list_entry {
    uint64_t data;              /* DEVICE address of pixel (0, 0) of the FRAME; filled by the caller, as is row_stride
                                   (bytes, >= 3 w) */
    int64_t  row_stride;
    int64_t  out_off;           /* byte offset of the entry's [oh][ow][3] output in the output buffer, a multiple of 16
                                   (the layout packs them; a caller may respace them and out_bytes) */
    int32_t  h, w;              /* the frame */
    int32_t  top, left, bh, bw; /* the box, inside the frame (the whole frame: 0, 0, h, w) */
    int32_t  oh, ow;            /* the output size */
    int32_t  ksx, ksy;          /* taps per output column / row (row length of the coefficient tables) */
    int32_t  bounds_x, coeffs_x, bounds_y, coeffs_y;   /* [ow][2] (first source index in the box, count), [ow][ksx]; [oh]... */
    int32_t  unit_rows;         /* output rows per work unit; 0: refused, no units, no tables */
    int32_t  chunk;             /* output columns per work unit (ow: the units keep the full width) */
} imgxf_resize_list_entry;
typedef struct imgxf_resize_list_unit {
    int32_t entry, y0, ny;      /* one workgroup: output rows [y0, y0 + ny) ... */
    int32_t x0, nx;             /* ... x output columns [x0, x0 + nx) of entry `entry` */
    int32_t col0, ncols;        /* the box columns the windows of those output columns touch: what the unit stages */
    int32_t lds_bytes;
} imgxf_resize_list_unit;
/* HOST half (no device work).  geometry: int32 [n][8] = (h, w, top, left, bh, bw, oh, ow) per entry; filter: any
 * IMGXF_RESAMPLE_*.  *block_bytes receives the block's size; block == NULL: only that.
 * Errors: IMGXF_ERR_NULL; IMGXF_ERR_ARG for n < 0, an unknown filter, lds_budget < 1, a side outside 1..32767, a box that
 * is empty or not inside its frame; IMGXF_ERR_SHAPE for a block beyond 2 GiB; IMGXF_ERR_WORKSPACE when block_cap is too
 * small. */
int imgxf_resize_list_layout_host(const int32_t* geometry, int n, int filter, int lds_budget, void* block, size_t block_cap,
                                  size_t* block_bytes);
/* The launch: block_host is the caller's host copy of the block, block_bytes its size, block_dev the same bytes on the
 * device (8-byte aligned), out the output buffer (16-byte aligned) of out_bytes bytes.  Before the launch every record is
 * checked against its frame, the block, the launch's LDS and the output buffer, so that they bound every address the
 * kernel forms (IMGXF_ERR_ARG / IMGXF_ERR_SHAPE / IMGXF_ERR_NULL, never a launch); nothing past block_bytes is read.  A
 * block without units launches nothing. */
int imgxf_resize_list_u8(const void* block_host, size_t block_bytes, const void* block_dev, void* out, size_t out_bytes,
                         void* stream);

/* ---- the transformations of apply_all_transformations on a LIST of entries over frames of different sizes -------------
 * The driver's eight types and the later driver's flip, crop + resize and perspective warp, each entry with its own
 * frame, type and drawn value, bit for bit what the per-type entry points give: one block
 *     imgxf_driver_header | imgxf_driver_entry[n] | imgxf_driver_unit[n_units] | int32 / float tables
 * laid out by the HOST, one copy of it to the device and at most three launches (the units that need no LDS, then the
 * perspective units with their fixed 32 KiB box, then the resample units of scale and crop + resize) plus one launch per
 * distinct (fixed, radius) among the blur entries — the drivers' grid has ten radii — whatever the number of frames,
 * entries or sizes.  A work unit is a band of output rows of one entry = one workgroup.
 * Blur is taken where the per-type dispatcher would serve a contiguous, 16-byte-aligned [n][h][w][3] batch of that size and
 * radius with the LDS-tiled kernel (csrc/sepconv_route.h: the planner of imgxf_sepconv_u8 itself), whose statements the blur units compile too (sepconv_tile.inc): the float Gaussian's
 * other kernel families agree with it to 1e-5, not to the byte, so those entries are refused (REFUSED_FAMILY) and keep
 * their own kernels.  The fixed-point evaluation is integer-exact in every family and is always taken. */
enum {
    IMGXF_DRIVER_SCALE = 0,          /* param[0] = factor: LANCZOS resize + centre crop (> 1) / paste on black (< 1) */
    IMGXF_DRIVER_ROTATION = 1,       /* param[0] = apply_rotation's angle: Image.rotate(-angle, NEAREST, fill black) */
    IMGXF_DRIVER_BRIGHTNESS = 2,     /* param[0] = ImageEnhance.Brightness's factor (1 + the drawn value) */
    IMGXF_DRIVER_CONTRAST = 3,       /* param[0] = cv2.convertScaleAbs's alpha (beta 0) */
    IMGXF_DRIVER_SHEAR = 4,          /* param[0] = shear factor: BICUBIC affine (1, sh, -ceil(sh h), 0, 1, 0), fill white */
    IMGXF_DRIVER_TRANSLATION = 5,    /* param[0], param[1] = tx, ty (moved by their integer parts, fill black) */
    IMGXF_DRIVER_NOISE = 6,          /* np.clip(frame + noise, 0, 255): float32 normals at imgxf_driver_entry.noise */
    IMGXF_DRIVER_FLIP = 7,           /* Image.transpose(FLIP_LEFT_RIGHT) */
    IMGXF_DRIVER_CROP_RESIZE = 8,    /* param[0], param[1] = x, y: the square window (x, y, x + cs, y + cs) with
                                        cs = int(0.78 w), resampled to 32 x 32 with BICUBIC; read in place */
    IMGXF_DRIVER_PERSPECTIVE = 10,   /* torchvision F.perspective(BILINEAR, fill 0) on the float tensor: eight float32
                                        coefficients at imgxf_driver_entry.pc (codes 9 and 11 are no type) */
    IMGXF_DRIVER_BLUR = 12,          /* param[0] = ksize, param[1] = sigma: imgxf_gaussian_u8 (cv2.GaussianBlur by its float
                                        definition, BORDER_REFLECT_101) */
    IMGXF_DRIVER_BLUR_FIXED = 13     /* param[0] = ksize, param[1] = sigma: imgxf_gaussian_cv_fixed_u8 (OpenCV's 8-bit
                                        fixed-point evaluation) */
};
enum {
    IMGXF_DRIVER_OK = 0,
    IMGXF_DRIVER_REFUSED_LDS = 1,    /* scale, crop: the source rows one output row touches do not fit lds_budget; blur: its
                                        (32 + 2 R) x 1024 bytes do not */
    IMGXF_DRIVER_REFUSED_SIZE = 2,   /* scale: the resized width or height would be below 1; crop: int(0.78 w) below 1;
                                        blur: ksize 0 (the drivers hand back the input itself) */
    IMGXF_DRIVER_REFUSED_TURN = 3,   /* rotation: Image.rotate's transpose paths (180, and 90 / 270 on square frames) */
    IMGXF_DRIVER_REFUSED_FORMAT = 4, /* the frame is not 3-channel uint8, or larger than 32767 x 32767 */
    IMGXF_DRIVER_REFUSED_OTHER = 5,  /* unknown type; a rotation whose rounded matrix is a pure scale (ImagingScaleAffine);
                                        a crop whose window is not inside the frame; a blur whose ksize is even, not in
                                        1 ... 31 or whose taps imgxf_gaussian_* would reject */
    IMGXF_DRIVER_REFUSED_FAMILY = 6  /* BLUR (float) only: the per-type dispatcher serves this size and radius with another
                                        kernel family than the LDS-tiled one */
};
typedef struct imgxf_driver_header {
    int32_t n_entries, n_units;
    int32_t n_plain;            /* units [0, n_plain) need no LDS (first launch); [n_plain, n_plain + n_persp) are the
                                   perspective units (second launch), then the resample units (third launch); the last
                                   n_blur units are the blur units */
    int32_t lds_bytes;          /* the largest resample unit's LDS need = the third launch's dynamic LDS size */
    int32_t entries_off, units_off, tables_off, total_bytes;   /* byte offsets of the sections, size of the block */
    uint64_t out_bytes;         /* size of the output allocation: every accepted entry's [oh][ow][3] at its out_off */
    int32_t n_persp;            /* perspective units: bands of 16 output rows, walked in 64-pixel tiles */
    int32_t n_blur;             /* blur units: bands of 32 output rows, walked in 256-byte column tiles; sorted by (fixed,
                                   radius), one launch per distinct pair */
} imgxf_driver_header;
typedef struct imgxf_driver_entry {
    uint64_t src;               /* DEVICE address of the frame's pixel (0, 0); filled by the caller, as is src_stride */
    int64_t  src_stride;        /* bytes between rows, >= 3 w */
    uint64_t noise;             /* IMGXF_DRIVER_NOISE: DEVICE address of h * w * 3 contiguous float32; filled by the caller */
    int64_t  out_off;           /* byte offset of the output (contiguous [oh][ow][3]) in the output allocation, 16-aligned */
    int32_t  op;                /* the device operation, IMGXF_DRIVER_*: a rotation by a multiple of 360 degrees is
                                   stated as a TRANSLATION by (0, 0), i.e. a copy */
    int32_t  status;            /* IMGXF_DRIVER_OK or the reason the entry has no units */
    int32_t  h, w, oh, ow;      /* source and output size */
    int32_t  unit_rows, frame;  /* output rows per work unit; the caller's frame index */
    float    alpha, beta;       /* BRIGHTNESS: blend factor; CONTRAST: alpha, beta */
    int32_t  dx, dy;            /* TRANSLATION; CROP_RESIZE: the window's corner (x, y) in the frame */
    int32_t  fx[6];             /* ROTATION: libImaging affine_fixed's 16.16 matrix of ops.rotate_matrix's coefficients */
    int32_t  win_top, win_left, win_h, win_w;   /* SCALE: where the resampled pixels go in the output (all of it for
                                   factors >= 1, the pasted window on the black canvas below 1); CROP_RESIZE: all of it */
    double   m1, m2;            /* SHEAR: the matrix (1, m1, m2, 0, 1, 0) */
    int32_t  ksx, ksy;          /* SCALE, CROP_RESIZE: taps per output column / row; BLUR: taps per axis, 2 R + 1 */
    int32_t  bounds_x, coeffs_x, bounds_y, coeffs_y;   /* [win_w][2], [win_w][ksx], [win_h][2], [win_h][ksy]: int32
                                   indices into the block; entries of equal (filter, in, out, window) on an axis share them.
                                   BLUR: coeffs_x / coeffs_y are the word indices of its ksx / ksy float taps (the fixed-point
                                   ones as n / 256); entries of equal (code, ksize, sigma) share one table */
    int32_t  row0, nrows, col0, ncols;   /* the rows / columns of the resampled region that the window touches */
    int32_t  in_h, in_w;        /* the resampled region, which the tables index: the frame for SCALE, the cs x cs window
                                   at (dx, dy) for CROP_RESIZE */
    float    pc[8];             /* PERSPECTIVE: torchvision's coefficients; filled by the caller, as src is */
} imgxf_driver_entry;
typedef struct imgxf_driver_unit {
    int32_t entry, y0, ny;      /* one workgroup: output rows [y0, y0 + ny) of entry `entry` */
    int32_t lds_bytes;          /* resample units: touched source rows x 12 ceil(win_w / 4) (rounded up to 16) + 4 staged
                                   row spans; blur units: (32 + 2 R) x 1024 */
} imgxf_driver_unit;
/* HOST half (no device work).  geometry: int32 [n][5] = (frame, type, h, w, channels; channels 0 = not uint8) per entry,
 * params: double [n][2].  Writes the block (block == NULL: only *block_bytes and the per-entry results) and, where
 * given, out_off [n] (-1 for a refused entry), out_hw [n][2], status [n], *out_bytes and *lds_bytes.  Lanczos tables are
 * precompute_coeffs' for (w -> int(w s)) and (h -> int(h s)), sliced to the centre-crop window for s > 1; a crop's are
 * the BICUBIC ones for (cs -> 32).  A resample unit takes up to 16 window rows, fewer where their touched source rows
 * would not fit half of lds_budget (three quarters, then all of it; capped at 64 KiB); a perspective unit takes 16 output
 * rows; a blur unit 32; the other units take the rows of about 24 KiB of output.  A blur's taps are those of
 * imgxf_gaussian_u8 / imgxf_gaussian_cv_fixed_u8 for (ksize, sigma), and whether it is taken follows the per-type
 * dispatcher's own choice of kernel family (IMGXF_NO_MARCH, IMGXF_MFMA_MIN_R and IMGXF_FX_MFMA_MIN_R included).
 * Errors: IMGXF_ERR_NULL; IMGXF_ERR_ARG for n < 0 or lds_budget < 1; IMGXF_ERR_SHAPE when the block or the output passes
 * 2 GiB / 2^40 bytes; IMGXF_ERR_WORKSPACE when block_cap is too small.  A refusal is a status, never an error. */
int imgxf_driver_list_layout_host(const int32_t* geometry, const double* params, int n, int lds_budget, void* block,
                                  size_t block_cap, size_t* block_bytes, int64_t* out_off, int32_t* out_hw, int32_t* status,
                                  size_t* out_bytes, int32_t* lds_bytes);
/* DEVICE half: copies block_host (checked first: IMGXF_ERR_ARG / IMGXF_ERR_SHAPE for a record that would let a kernel
 * leave its frame, the output or the block, or for a perspective coefficient that is not finite) to block_dev (8-byte
 * aligned, total_bytes) on the stream and launches.  out: the output allocation (16-byte aligned, out_cap >= out_bytes).  No allocation, no synchronisation. */
int imgxf_driver_list_u8(const void* block_host, void* block_dev, uint8_t* out, size_t out_cap, void* stream);

/* ---- apply_background_change on a LIST of RGB frames of different sizes, each with its own colour, in two launches -----
 * Entry k is bit for bit
 *     Image.composite(img, Image.new("RGB", img.size, colour_k),
 *                     Image.fromarray(binary_dilation(e > np.percentile(e, q), iterations=3)))
 *     with e = ndimage.sobel(np.array(img.convert("L")))
 * — what imgxf_rgb_sobel_u8 (X_WRAP), imgxf_histogram_u8, imgxf_percentile_mask_u8, imgxf_dilate_cross_u8 (3) and
 * imgxf_composite_const_u8 give in five calls — for uint8 RGB frames from 1 x 1 up, rows at any stride and byte offset,
 * read in place.  One host block
 *     imgxf_background_list_header | imgxf_background_list_entry[n] | imgxf_background_list_unit[n_units]
 * one copy of it to the device, one hipMemsetAsync of the histogram workspace (hist_bytes, never uploaded) and two
 * launches whatever the number of frames or sizes.  A work unit is one tile_h x tile_w tile of one entry, the units of
 * an entry in row-major order, the entries in order.  Launch 1 counts the x-Sobel bytes of its tiles (staged with a
 * one-pixel halo, no edge plane is stored) into the entry's uint32[256] histogram; launch 2 recomputes the edges of a
 * tile plus a halo of 3, takes the entry's threshold from that histogram with the float64 statements of
 * imgxf_percentile_mask_u8, dilates e > threshold (0 outside the image) to L1 distance 3 in LDS and stores
 * mask ? rgb : colour.  The bytes do not depend on where a tile lies or on the width modulo anything. */
typedef struct imgxf_background_list_header {
    int32_t n_entries, n_units;
    int32_t entries_off, units_off, total_bytes;   /* byte offsets of the sections, size of the block */
    int32_t tile_h, tile_w;     /* imgxf_background_list_tile's, which the units were cut for */
    int32_t pad_;
    int64_t out_bytes;          /* size of the output buffer: the end of the last entry's slot */
    int64_t hist_bytes;         /* size of the histogram workspace: 1024 n_entries */
} imgxf_background_list_header;
typedef struct imgxf_background_list_entry {
    uint64_t data;              /* DEVICE address of pixel (0, 0) of the frame; filled by the caller, as is row_stride
                                   (bytes, >= 3 w) */
    int64_t  row_stride;
    int64_t  out_off;           /* byte offset of the entry's [h][w][3] output in the output buffer, a multiple of 16
                                   (the layout packs them; a caller may respace them and out_bytes) */
    int64_t  hist_off;          /* byte offset of the entry's uint32[256] in the workspace: 1024 k */
    int32_t  h, w;
    uint8_t  colour[4];         /* r, g, b, 0 */
    int32_t  first_unit;        /* index of the entry's first work unit */
} imgxf_background_list_entry;
typedef struct imgxf_background_list_unit {
    int32_t entry, y0, x0;      /* one tile: rows [y0, y0 + tile_h) x columns [x0, x0 + tile_w) of entry `entry`, cut
                                   at the frame */
} imgxf_background_list_unit;
/* The tile of a work unit, for callers and tests that place content on tile seams. */
int imgxf_background_list_tile(int* tile_h, int* tile_w);
/* HOST half (no device work).  geometry: int32 [n][5] = (h, w, r, g, b) per entry.  *block_bytes receives the block's
 * size; block == NULL: only that.  Errors: IMGXF_ERR_NULL; IMGXF_ERR_ARG for n < 0, a side outside 1..32767, a colour
 * byte outside 0..255; IMGXF_ERR_SHAPE for a block beyond 2 GiB; IMGXF_ERR_WORKSPACE when block_cap is too small. */
int imgxf_background_list_layout_host(const int32_t* geometry, int n, void* block, size_t block_cap, size_t* block_bytes);
/* The launches: block_host is the caller's host copy of the block, block_bytes its size, block_dev the same bytes on the
 * device (8-byte aligned), out the output buffer (16-byte aligned) of out_bytes bytes, q the percentile in 0..100 (the
 * reference: 70), workspace a device buffer (4-byte aligned) of workspace_bytes >= hist_bytes that the call zeroes.
 * Dilation iterations are the reference's 3.  Before any device work every record is checked against its frame, the
 * block, the workspace and the output buffer, and the units against the one tiling of their entries, so that they
 * bound every address the kernels form (IMGXF_ERR_ARG / IMGXF_ERR_SHAPE / IMGXF_ERR_NULL, never a launch); nothing past
 * block_bytes is read.  A block without units launches nothing.  No allocation, no synchronisation. */
int imgxf_background_list_u8(const void* block_host, size_t block_bytes, const void* block_dev, void* out, size_t out_bytes,
                             double q, void* workspace, size_t workspace_bytes, void* stream);
/* Device work the last imgxf_background_list_u8 of this thread queued: counts[0] kernel launches, counts[1] memsets
 * (for tests of the two-launch contract). */
int imgxf_background_list_last_counts(int* counts);

/* ---- Image.transform(size, AFFINE, m, resample, fillcolor) on a LIST of RGB frames of different sizes -----------------
 * Entry k is bit for bit Image.fromarray(frame).transform((ow, oh), Image.AFFINE, m_k, filter_k, fillcolor=fill_k): every
 * entry with its own frame, matrix, output size, filter (NEAREST, BILINEAR, BICUBIC, mixed freely in one call) and fill,
 * uint8 RGB in and out, rows of the frames at any stride and byte offset, read in place; several entries may read one
 * frame.  The HOST lays out one block
 *     imgxf_affine_list_header | imgxf_affine_list_entry[n] | imgxf_affine_list_unit[n_units] | int32 tables
 * which the caller copies to the device once.  The outputs are [oh][ow][3] uint8, contiguous, each at its entry's out_off
 * (a multiple of 16) in ONE output buffer of out_bytes bytes.
 *
 * An entry takes one of four ROUTES, libImaging's own three NEAREST / filter paths less the one it is refused for:
 *   SCALE     NEAREST with m1 == m3 == 0 (ImagingScaleAffine): per entry the tables xin[ow] at xtab and yin[oh] at ytab
 *             (int32 indices into the block), built by the running double additions xo = m2 + m0 * 0.5; xo += m0 and
 *             COORD(v) = v < 0 ? -1 : (int)v (stored as INT32_MAX from 2^31 up); [xmin, xmax) is the span of output columns
 *             whose source column lies in the frame — the span libImaging copies; rows test their own yin;
 *   FIXED     NEAREST otherwise (affine_fixed): fx[6] is the matrix in 16.16 fixed point, the half-pixel offsets folded
 *             into fx[2] and fx[5], int arithmetic that wraps as C's does.  libImaging takes this path only where
 *             |x m0 + y m1 + m2| < 32768 and |x m3 + y m4 + m5| < 32768 at (0, 0), (ow, 0), (0, oh), (ow, oh) and runs a
 *             float loop elsewhere: such an entry is REFUSED by the layout (IMGXF_ERR_UNSUPPORTED), never served in
 *             fixed point; so is one with a coefficient of magnitude 32768 or more, which no 16.16 int holds (C leaves
 *             that conversion undefined);
 *   BILINEAR  coordinates m0 (x + 0.5) + m1 (y + 0.5) + m2 in un-contracted fp64, the inside test on the doubles, clamped
 *   BICUBIC   neighbours, libImaging's BILINEAR / BICUBIC macros in fp64 for every pixel, (UINT8)v truncation (BICUBIC
 *             clipped first).
 * A work unit is one tile of at most IMGXF_AFFINE_LIST_TILE_W x IMGXF_AFFINE_LIST_TILE_H output pixels of one entry (cut
 * at the output's right and bottom edge) = one 256-lane workgroup, each lane four consecutive pixels of one row: a
 * rotated gather of whole rows would have no locality.  The units are sorted by route (in the order above; within a
 * route by entry, then row-major) and the header states each route's first unit and count: one launch per route present,
 * four at most, so that NEAREST does not carry the registers of the fp64 routes. */
enum {
    IMGXF_AFFINE_LIST_SCALE = 0, IMGXF_AFFINE_LIST_FIXED = 1, IMGXF_AFFINE_LIST_BILINEAR = 2, IMGXF_AFFINE_LIST_BICUBIC = 3,
    IMGXF_AFFINE_LIST_ROUTES = 4
};
#define IMGXF_AFFINE_LIST_TILE_W 64
#define IMGXF_AFFINE_LIST_TILE_H 16
typedef struct imgxf_affine_list_header {
    int32_t n_entries, n_units;
    int32_t entries_off, units_off, tables_off, total_bytes;   /* byte offsets of the sections, size of the block */
    int32_t route_first[IMGXF_AFFINE_LIST_ROUTES];              /* units [route_first[r], route_first[r] + route_count[r]) */
    int32_t route_count[IMGXF_AFFINE_LIST_ROUTES];              /* are route r's; the ranges follow each other from 0 */
    int64_t out_bytes;          /* size of the output buffer: the end of the last entry's slot */
} imgxf_affine_list_header;
typedef struct imgxf_affine_list_entry {
    uint64_t data;              /* DEVICE address of pixel (0, 0) of the frame; filled by the caller, as is row_stride
                                   (bytes, >= 3 w) */
    int64_t  row_stride;
    int64_t  out_off;           /* byte offset of the entry's [oh][ow][3] output in the output buffer, a multiple of 16
                                   (the layout packs them; a caller may respace them and out_bytes) */
    int32_t  h, w;              /* the frame */
    int32_t  oh, ow;            /* the output size */
    int32_t  route;             /* IMGXF_AFFINE_LIST_* */
    int32_t  xtab, ytab;        /* SCALE: word indices of xin[ow] and yin[oh]; 0 on the other routes */
    int32_t  xmin, xmax;        /* SCALE: the output columns [xmin, xmax) have a source column inside the frame */
    uint8_t  fill[4];           /* r, g, b, 0 */
    double   m[6];              /* the matrix as the caller gave it (BILINEAR, BICUBIC read it) */
    int32_t  fx[6];             /* FIXED: affine_fixed's 16.16 matrix; 0 on the other routes */
} imgxf_affine_list_entry;
typedef struct imgxf_affine_list_unit {
    int32_t entry, x0, y0;      /* one tile: columns [x0, x0 + TILE_W) x rows [y0, y0 + TILE_H) of entry `entry`, cut at
                                   the output's edges; x0 and y0 are multiples of the tile's sides */
} imgxf_affine_list_unit;
/* HOST half (no device work).  geometry: int32 [n][4] = (h, w, oh, ow) per entry; matrices: double [n][6]; filters: int32
 * [n] of IMGXF_FILTER_*; fills: uint8 [n][3].  *block_bytes receives the block's size; block == NULL: only that.
 * Errors: IMGXF_ERR_NULL; IMGXF_ERR_ARG for n < 0, a side outside 1..32767, an unknown filter, a matrix coefficient that is
 * not finite; IMGXF_ERR_UNSUPPORTED for a NEAREST entry that libImaging takes out of 16.16 fixed point or that does not fit it (above);
 * IMGXF_ERR_SHAPE for a block beyond 2 GiB; IMGXF_ERR_WORKSPACE when block_cap is too small. */
int imgxf_affine_list_layout_host(const int32_t* geometry, const double* matrices, const int32_t* filters, const uint8_t* fills,
                                  int n, void* block, size_t block_cap, size_t* block_bytes);
/* The launches: block_host is the caller's host copy of the block, block_bytes its size, block_dev the same bytes on the
 * device (8-byte aligned), out the output buffer (16-byte aligned) of out_bytes bytes.  Before any launch every record and
 * unit is checked against its frame, the block, the tables and the output buffer, so that they bound every address the
 * kernels form (IMGXF_ERR_ARG / IMGXF_ERR_SHAPE / IMGXF_ERR_NULL, never a launch); nothing past block_bytes is read.  At
 * most one launch per route present; a block without units launches nothing.  No allocation, no synchronisation. */
int imgxf_affine_list_u8(const void* block_host, size_t block_bytes, const void* block_dev, void* out, size_t out_bytes,
                         void* stream);
/* Kernel launches the last imgxf_affine_list_u8 of this thread queued (for tests of the launch count). */
int imgxf_affine_list_last_launches(int* launches);

/* ---- Image.transform(size, PERSPECTIVE | QUAD, data, resample, fillcolor) on a LIST of RGB frames of different sizes ---
 * Entry k is bit for bit Image.fromarray(frame).transform((ow, oh), method_k, a_k, filter_k, fillcolor=fill_k): every entry
 * with its own frame, method, eight coefficients, output size, filter (NEAREST, BILINEAR, BICUBIC) and fill, all mixed
 * freely in one call; frames, outputs and the block protocol as for the affine list above.  The HOST lays out one block
 *     imgxf_transform_list_header | imgxf_transform_list_entry[n] | imgxf_transform_list_unit[n_units]
 * (no tables: tables_off states the end of the units).
 *
 * The statements are libImaging's ImagingGenericTransform (Geometry.c), every operation rounded on its own in fp64, at
 * the pixel centre xin = x + 0.5, yin = y + 0.5:
 *   PERSPECTIVE  d = (a6 xin + a7 yin) + 1;  xs = ((a0 xin + a1 yin) + a2) / d;  ys = ((a3 xin + a4 yin) + a5) / d
 *   QUAD         xs = ((a0 + a1 xin) + a2 yin) + (a3 xin) yin;  ys = ((a4 + a5 xin) + a6 yin) + (a7 xin) yin
 *                (a: what Image.transform's Python layer makes of the four corners, not the corners themselves)
 *   NEAREST      COORD(v) = v < 0 ? -1 : (int)v on xs and ys (from 2^31 up: outside), then the in-frame test;
 *   BILINEAR,    the in-frame test 0 <= xs < w && 0 <= ys < h on the doubles, then libImaging's fp64 filters as on the
 *   BICUBIC      affine list.
 * A pixel that fails its test is the entry's fill.  The ROUTE of an entry is 3 method + filter: six kernels, so that
 * NEAREST does not carry the registers of the fp64 filters and PERSPECTIVE alone carries the divisions.
 *
 * REFUSED (IMGXF_ERR_UNSUPPORTED), because libImaging's own result is not defined there: a coefficient of magnitude above
 * IMGXF_TRANSFORM_LIST_MAX_COEFF — below it no product or sum of the statements overflows at sides up to 32767
 * (|a xin yin| <= 1e290 * 32767^2 < 1.1e299, four such terms < DBL_MAX) — and a PERSPECTIVE entry whose denominator d,
 * evaluated by the statements above, is not strictly of one sign at the four corner pixel centres (0.5 | ow - 0.5,
 * 0.5 | oh - 0.5): the warp's horizon crosses the output.  Every rounded step of d is monotone in xin and in yin, so the
 * corners bound d at every pixel: a served entry never divides by zero and never makes a NaN. */
enum { IMGXF_TRANSFORM_PERSPECTIVE = 0, IMGXF_TRANSFORM_QUAD = 1, IMGXF_TRANSFORM_METHODS = 2 };
#define IMGXF_TRANSFORM_LIST_ROUTES 6          /* route = 3 * method + IMGXF_FILTER_* (NEAREST 0, BILINEAR 1, BICUBIC 2) */
#define IMGXF_TRANSFORM_LIST_TILE_W 64
#define IMGXF_TRANSFORM_LIST_TILE_H 16
#define IMGXF_TRANSFORM_LIST_MAX_COEFF 1e290
typedef struct imgxf_transform_list_header {
    int32_t n_entries, n_units;
    int32_t entries_off, units_off, tables_off, total_bytes;   /* byte offsets of the sections (tables_off: the end of the
                                                                   units), size of the block */
    int32_t route_first[IMGXF_TRANSFORM_LIST_ROUTES];           /* units [route_first[r], route_first[r] + route_count[r]) */
    int32_t route_count[IMGXF_TRANSFORM_LIST_ROUTES];           /* are route r's; the ranges follow each other from 0 */
    int64_t out_bytes;          /* size of the output buffer: the end of the last entry's slot */
} imgxf_transform_list_header;
typedef struct imgxf_transform_list_entry {
    uint64_t data;              /* DEVICE address of pixel (0, 0) of the frame; filled by the caller, as is row_stride
                                   (bytes, >= 3 w) */
    int64_t  row_stride;
    int64_t  out_off;           /* byte offset of the entry's [oh][ow][3] output in the output buffer, a multiple of 16
                                   (the layout packs them; a caller may respace them and out_bytes) */
    int32_t  h, w;              /* the frame */
    int32_t  oh, ow;            /* the output size */
    int32_t  route;             /* 3 * IMGXF_TRANSFORM_* + IMGXF_FILTER_* */
    uint8_t  fill[4];           /* r, g, b, 0 */
    double   a[8];              /* the coefficients as the caller gave them */
} imgxf_transform_list_entry;
typedef struct imgxf_transform_list_unit {
    int32_t entry, x0, y0;      /* one tile: columns [x0, x0 + TILE_W) x rows [y0, y0 + TILE_H) of entry `entry`, cut at
                                   the output's edges; x0 and y0 are multiples of the tile's sides */
} imgxf_transform_list_unit;
/* HOST half (no device work).  geometry: int32 [n][4] = (h, w, oh, ow) per entry; methods: int32 [n] of IMGXF_TRANSFORM_*;
 * coeffs: double [n][8]; filters: int32 [n] of IMGXF_FILTER_*; fills: uint8 [n][3].  *block_bytes receives the block's size;
 * block == NULL: only that.  Errors: IMGXF_ERR_NULL for a null argument; IMGXF_ERR_ARG for n < 0, a side outside 1..32767, an
 * unknown method or filter, a coefficient that is not finite; IMGXF_ERR_UNSUPPORTED for a coefficient above
 * IMGXF_TRANSFORM_LIST_MAX_COEFF in magnitude or a PERSPECTIVE denominator that is zero at a corner pixel centre or changes
 * sign between two (above); IMGXF_ERR_SHAPE for a block beyond 2 GiB or more than 2^31 - 1 units; IMGXF_ERR_WORKSPACE when
 * block_cap is too small. */
int imgxf_transform_list_layout_host(const int32_t* geometry, const int32_t* methods, const double* coeffs, const int32_t* filters,
                                     const uint8_t* fills, int n, void* block, size_t block_cap, size_t* block_bytes);
/* The launches: block_host is the caller's host copy of the block, block_bytes its size, block_dev the same bytes on the
 * device (8-byte aligned), out the output buffer (16-byte aligned) of out_bytes bytes.  Before any launch every record and
 * unit is checked: IMGXF_ERR_NULL for a null block or a frame without an address; IMGXF_ERR_SHAPE for a frame or an output
 * with a side outside 1..32767 or a row_stride below 3 w; IMGXF_ERR_ARG for sections that do not follow from the counts
 * or leave the block, route ranges that do not follow each other and cover the units, an unknown route, an output slot
 * that is misaligned or leaves the buffer, a unit outside its entry, off the tile grid or in another route's range, or a
 * misaligned device pointer; IMGXF_ERR_UNSUPPORTED for coefficients the layout would have refused.  None of them launches
 * anything, and nothing past block_bytes is read.  At most one launch per route present, six at most; a block without
 * units launches nothing.  No allocation, no synchronisation. */
int imgxf_transform_list_u8(const void* block_host, size_t block_bytes, const void* block_dev, void* out, size_t out_bytes,
                            void* stream);
/* Kernel launches the last imgxf_transform_list_u8 of this thread queued (for tests of the launch count). */
int imgxf_transform_list_last_launches(int* launches);

#ifdef __cplusplus
}
#endif
#endif /* IMGXF_H */
