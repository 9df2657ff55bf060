// JPEG compression applied to frames that stay on the device (included by jpeg.hip inside namespace imgxf): the pixels of
// `Image.open(f).convert("RGB")` after `Image.fromarray(frame).save(f, "JPEG", quality=q, subsampling=s)`, without a file.
// Entropy coding is lossless, so the pixels are fixed by the forward half of the writer's transform stage and the inverse
// half of the reader; the fused kernels are the writer's transform kernels with another SINK:
//
//   jpeg_transform_kernel<W, JpegPlaneSink>        4:2:0, a uniform batch or a list of frames of different sizes: staging,
//   jpeg_transform_ex_kernel<L, JpegPlaneSink>     colour conversion and downsampling are the writer's own statements, and
//   jpeg_transform_ex_kernel<JLGRAY, JpegGraySink> so are jpeg_forward_block's (fdct8 twice, the quantiser).  The thread
//                                                  that holds the block's 64 quantised values then multiplies them by the
//                                                  quantiser steps, runs the reader's idct8 over columns and rows and its
//                                                  range limit (jpeg_idct.h) — all in registers — and stores 8 × 8 samples.
//                                                  No coefficient, DC difference or bit count reaches memory.
//
// Colour frames: the samples go to component planes in the reader's layout (pitch blocks_x · 8, planes padded to whole
// MCUs), because fancy upsampling needs one chroma sample beyond a strip on every side; the reader's own colour stage
// (imgxf_jpeg_decode_color: sample_at + jdcolor.c) then reads them through the imgxf_jpeg_dec_image records the host
// builds here.  Grayscale frames are their one plane: the sink writes the destination directly, clipped to the frame.
// Blocks the writer only codes as dummies (past the last real block row / column) are never read by the colour stage and
// are not written.

// jdct.h DEQUANTIZE, then jidctint.c jpeg_idct_islow: columns (the result scaled up by 4), rows, the range limit; row r of
// the block as eight bytes in rows[r].
// (idct8's multiplies stay the reader's plain ones: with explicit 24-bit instructions, like the forward passes', the 1024-frame
// batch of profiles/jpeg_roundtrip.txt took the same 2.06 ms between device events in alternating runs)
__device__ __forceinline__ void jpeg_reconstruct_block(int (&d)[64], int chroma, const JpegQuant& q, uint2 (&rows)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int x[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = d[r * 8 + c] * (int)q.step[chroma][r * 8 + c];
        idct8(x, o, IDCT_SHIFT_COLUMNS);
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r * 8 + c] = o[r];
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int x[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = d[r * 8 + k];
        idct8(x, o, IDCT_SHIFT_ROWS);
        u32 lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= range_limit_centered(o[k]) << (8 * k);
            hi |= range_limit_centered(o[k + 4]) << (8 * k);
        }
        rows[r] = make_uint2(lo, hi);
    }
}

// Colour frames: block (bx, by) of component comp into the component's plane, as the record of frame f lays it out
// (plane_off and the pitch are multiples of 8: whole aligned rows).
struct JpegPlaneSink {
    static constexpr bool CODES = false;
    __device__ __forceinline__ int64_t coef_offset(int) const { return 0; }
    __device__ __forceinline__ int64_t blk_offset(int) const { return 0; }
    u8* __restrict__ planes;
    const imgxf_jpeg_dec_image* __restrict__ images;
    struct Where {                                               // (read from the record before the transform: the loads hide behind it)
        u8* dst;
        int64_t pitch;
    };
    __device__ __forceinline__ Where locate(const JpegBlockAt& at) const {
        const imgxf_jpeg_dec_comp& cp = images[at.f].comp[at.comp];
        const int64_t pitch = (int64_t)cp.blocks_x * 8;
        return {planes + cp.plane_off + (int64_t)at.by * 8 * pitch + at.bx * 8, pitch};
    }
    __device__ __forceinline__ void operator()(int (&d)[64], int chroma, const JpegQuant& q, const u8 (*)[256], const Where& w) const {
        uint2 rows[8];
        jpeg_reconstruct_block(d, chroma, q, rows);
#pragma unroll
        for (int r = 0; r < 8; ++r) *(uint2*)(w.dst + r * w.pitch) = rows[r];
    }
};

// Grayscale frames: the block straight into frame f of the destination view, rows and columns past the frame dropped.
struct JpegGraySink {
    static constexpr bool CODES = false;
    __device__ __forceinline__ int64_t coef_offset(int) const { return 0; }
    __device__ __forceinline__ int64_t blk_offset(int) const { return 0; }
    View dst;
    struct Where {
        u8* base;
        int x0, y0;
    };
    __device__ __forceinline__ Where locate(const JpegBlockAt& at) const {
        const int x0 = at.bx * 8, y0 = at.by * 8;
        return {dst.p + (int64_t)at.f * dst.fs + (int64_t)y0 * dst.rs + x0, x0, y0};
    }
    __device__ __forceinline__ void operator()(int (&d)[64], int chroma, const JpegQuant& q, const u8 (*)[256], const Where& w) const {
        uint2 rows[8];
        jpeg_reconstruct_block(d, chroma, q, rows);
        const int x0 = w.x0, y0 = w.y0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (y0 + r >= dst.h) break;
            u8* p = w.base + (int64_t)r * dst.rs;
            if (x0 + 8 <= dst.w && (((uintptr_t)p) & 7) == 0) {
                *(uint2*)p = rows[r];
            } else {
#pragma unroll
                for (int b = 0; b < 8; ++b)
                    if (x0 + b < dst.w) p[b] = (u8)((b < 4 ? rows[r].x : rows[r].y) >> (8 * (b & 3)));
            }
        }
    }
};

// ---- host side ------------------------------------------------------------------------------------------------------

// The record the reader's colour stage reads for an h × w frame written in layout `lay` (what imgxf_jpeg_layout_host
// reports for the file: MCU-padded planes one after the other from plane_o on); returns the bytes of the frame's planes.
static int64_t rt_describe(imgxf_jpeg_dec_image& im, int lay, int h, int w, int index, int64_t plane_o, int64_t out_off, int64_t out_pitch) {
    memset(&im, 0, sizeof(im));
    const int hs = lay == JL444 ? 1 : 2, vs = lay == JL420 ? 2 : 1;
    im.width = w; im.height = h; im.ncomp = 3; im.hmax = hs; im.vmax = vs;
    im.mcux = (w + 8 * hs - 1) / (8 * hs);
    im.mcuy = (h + 8 * vs - 1) / (8 * vs);
    im.restart_interval = im.mcux * im.mcuy;                   // no restart markers: one segment (unused here: there is no stream)
    im.seg_first = index; im.seg_count = 1;
    im.out_off = out_off; im.out_pitch = out_pitch;
    int64_t pos = plane_o;
    for (int c = 0; c < 3; ++c) {
        imgxf_jpeg_dec_comp& cp = im.comp[c];
        cp.h = c ? 1 : hs; cp.v = c ? 1 : vs;
        cp.dc_tab = cp.ac_tab = cp.quant = c ? 1 : 0;
        cp.blocks_x = im.mcux * cp.h; cp.blocks_y = im.mcuy * cp.v;
        cp.dw = (w * cp.h + hs - 1) / hs; cp.dh = (h * cp.v + vs - 1) / vs;
        cp.coef_off = 0;                                       // no coefficient reaches memory
        cp.plane_off = pos;
        pos += (int64_t)cp.blocks_x * cp.blocks_y * 64;
    }
    return pos - plane_o;
}

// only the sampling decides a pixel: optimize (0 / 1) is accepted and ignored
static int rt_layout(const imgxf_jpeg_enc_params* p) { return enc_layout(p); }

static int rt_workspace(int lay, int n, int h, int w, size_t* rec_bytes, size_t* plane_fs) {
    if (n < 0 || n > 65535 || h < 1 || w < 1 || h > 32767 || w > 32767) return IMGXF_ERR_SHAPE;
    *rec_bytes = *plane_fs = 0;
    if (lay == JLGRAY) return IMGXF_OK;                        // the sink writes the destination: nothing to stage
    imgxf_jpeg_dec_image im;
    *plane_fs = (size_t)rt_describe(im, lay, h, w, 0, 0, 0, 0);
    *rec_bytes = al256((size_t)n * sizeof(imgxf_jpeg_dec_image));
    return IMGXF_OK;
}

// The records of a uniform batch's n frames (imgxf_jpeg_roundtrip_records_host; what rt_uniform copies to the head of its
// workspace): frame f's planes from f · (the frame's plane bytes) on, its pixels at f · out_frame_stride.
static int rt_records(int lay, int n, int h, int w, int64_t out_row_stride, int64_t out_frame_stride, imgxf_jpeg_dec_image* images) {
    size_t rec_bytes, plane_fs;
    IMGXF_CHECK(rt_workspace(lay, n, h, w, &rec_bytes, &plane_fs));
    for (int f = 0; f < n; ++f) rt_describe(images[f], lay, h, w, f, (int64_t)f * (int64_t)plane_fs, (int64_t)f * out_frame_stride, out_row_stride);
    return IMGXF_OK;
}

// A list's block: imgxf_jpeg_roundtrip_list_header | imgxf_jpeg_list_frame[n] | imgxf_jpeg_dec_image[n] | the transform
// stage's unit table.  Of a frame record only the geometry (h .. nblk) and its output slot are used; the planes' offsets
// are the decoder record's.  block == nullptr: the sizes alone.
static_assert(sizeof(imgxf_jpeg_roundtrip_list_header) == 40, "include/imgxf.h documents this record");
static int rt_list_build(int n, const int32_t* sizes, u8* block, size_t block_cap, imgxf_jpeg_roundtrip_list_header* out_hd) {
    if (n < 0 || n > 65535) return IMGXF_ERR_SHAPE;
    imgxf_jpeg_roundtrip_list_header hd;
    memset(&hd, 0, sizeof(hd));
    hd.n_frames = n;
    hd.frames_off = (int32_t)sizeof(hd);
    std::vector<imgxf_jpeg_list_frame> fr((size_t)n);
    std::vector<imgxf_jpeg_dec_image> im((size_t)n);
    size_t units = 0, out = 0;
    int64_t planes = 0;
    for (int i = 0; i < n; ++i) {
        const int h = sizes[2 * i], w = sizes[2 * i + 1];
        if (h < 1 || w < 1 || h > 32767 || w > 32767) return IMGXF_ERR_SHAPE;
        imgxf_jpeg_list_frame& f = fr[(size_t)i];
        memset(&f, 0, sizeof(f));
        f.h = h; f.w = w;
        f.mw = (w + 15) / 16; f.mh = (h + 15) / 16; f.bw = (w + 7) / 8; f.bh = (h + 7) / 8;
        f.nblk = f.mw * f.mh * 6;
        f.out_off = (int64_t)out;
        f.out_cap = (int64_t)h * w * 3;
        planes += rt_describe(im[(size_t)i], JL420, h, w, i, planes, f.out_off, (int64_t)w * 3);
        out += ((size_t)f.out_cap + 15) & ~(size_t)15;
        units += (size_t)list_stage_units(f, 0);
    }
    hd.workspace_bytes = (uint64_t)planes;
    hd.out_bytes = out;
    size_t pos = sizeof(hd) + (size_t)n * sizeof(imgxf_jpeg_list_frame);
    hd.images_off = (int32_t)pos;
    pos += (size_t)n * sizeof(imgxf_jpeg_dec_image);
    if (units > 0x7fffffffu || pos + units * sizeof(imgxf_jpeg_list_unit) > 0x7fffffffu) return IMGXF_ERR_ARG;
    hd.units_off = (int32_t)pos;
    hd.n_units = (int32_t)units;
    pos += units * sizeof(imgxf_jpeg_list_unit);
    hd.total_bytes = (int32_t)pos;
    *out_hd = hd;
    if (!block) return IMGXF_OK;
    if (block_cap < pos) return IMGXF_ERR_WORKSPACE;
    memcpy(block, &hd, sizeof(hd));
    if (n) {
        memcpy(block + hd.frames_off, fr.data(), (size_t)n * sizeof(imgxf_jpeg_list_frame));
        memcpy(block + hd.images_off, im.data(), (size_t)n * sizeof(imgxf_jpeg_dec_image));
    }
    u8* up = block + hd.units_off;                             // (byte copies: the caller's block may sit at any address)
    for (int i = 0; i < n; ++i) {
        const imgxf_jpeg_list_frame& f = fr[(size_t)i];
        const int ngx = (f.mw + JM - 1) / JM;
        for (int my = 0; my < f.mh; ++my)
            for (int gx = 0; gx < ngx; ++gx) {
                const imgxf_jpeg_list_unit u = {i, gx | (my << 16)};
                memcpy(up, &u, sizeof(u));
                up += sizeof(u);
            }
    }
    return IMGXF_OK;
}

static int rt_uniform(const imgxf_view* src, const imgxf_view* dst, const imgxf_jpeg_enc_params* params, const imgxf_jpeg_tables* tables,
                      void* workspace, size_t workspace_bytes, void* stream) {
    IMGXF_CHECK(check_view(src));
    IMGXF_CHECK(check_view(dst));
    if (!params || !tables) return IMGXF_ERR_NULL;
    const int lay = rt_layout(params);
    if (lay < 0) return IMGXF_ERR_ARG;
    if (src->c != params->ncomp) return IMGXF_ERR_UNSUPPORTED;
    if (!same_geometry(src, dst)) return IMGXF_ERR_SHAPE;
    if (src->n == 0) return IMGXF_OK;
    if (empty_view(src)) return IMGXF_ERR_SHAPE;
    size_t rec_bytes, plane_fs;
    IMGXF_CHECK(rt_workspace(lay, src->n, src->h, src->w, &rec_bytes, &plane_fs));
    const size_t need = rec_bytes + (size_t)src->n * plane_fs;
    if (need && (!workspace || workspace_bytes < need || (((uintptr_t)workspace) & 15))) return IMGXF_ERR_WORKSPACE;
    JpegQuant q;
    IMGXF_CHECK(jpeg_prepare_quant(q, tables, params->ncomp));
    const View s = make_view(src), d = make_view(dst);
    const int n = s.n;
    hipStream_t st = (hipStream_t)stream;
    const JpegLayout G = jpeg_layout(lay, false, false, 1, s.h, s.w, 4096);   // the geometry alone (mw, mh, bw, bh)
    if (lay == JLGRAY) {
        const int per = JXP / JLay<JLGRAY>::MW;
        hipLaunchKernelGGL((jpeg_transform_ex_kernel<JLGRAY, JpegGraySink, JpegUniform>),
                           dim3((unsigned)((G.mw + per - 1) / per), (unsigned)G.mh, (unsigned)n), dim3(JLay<JLGRAY>::T), 0, st, s, JpegGraySink{d}, G.mw,
                           G.bw, q, JpegUniform{});
        return launch_status();
    }
    std::vector<imgxf_jpeg_dec_image> im;
    try {
        im.resize((size_t)n);
    } catch (const std::bad_alloc&) {
        return IMGXF_ERR_WORKSPACE;
    }
    IMGXF_CHECK(rt_records(lay, n, s.h, s.w, d.rs, d.fs, im.data()));
    u8* ws = (u8*)workspace;
    const imgxf_jpeg_dec_image* images = (const imgxf_jpeg_dec_image*)ws;
    u8* planes = ws + rec_bytes;
    // (pageable host memory: hipMemcpyAsync has copied it to the runtime's staging memory when it returns, so the vector
    // may go; include/imgxf.h states what that means for the caller)
    const hipError_t ce = hipMemcpyAsync(ws, im.data(), (size_t)n * sizeof(imgxf_jpeg_dec_image), hipMemcpyHostToDevice, st);
    if (ce != hipSuccess) return (int)ce;
    const JpegPlaneSink sink = {planes, images};
    if (lay == JL420) {
        hipLaunchKernelGGL((jpeg_transform_kernel<JpegUniform, JpegPlaneSink>), dim3((unsigned)((G.mw + JM - 1) / JM), (unsigned)G.mh, (unsigned)n),
                           dim3(JT), 0, st, s, sink, G.mw, G.bw, G.bh, q, JpegUniform{});
    } else if (lay == JL422) {
        const int per = JXP / JLay<JL422>::MW;
        hipLaunchKernelGGL((jpeg_transform_ex_kernel<JL422, JpegPlaneSink, JpegUniform>),
                           dim3((unsigned)((G.mw + per - 1) / per), (unsigned)G.mh, (unsigned)n), dim3(JLay<JL422>::T), 0, st, s, sink, G.mw,
                           G.bw, q, JpegUniform{});
    } else {
        const int per = JXP / JLay<JL444>::MW;
        hipLaunchKernelGGL((jpeg_transform_ex_kernel<JL444, JpegPlaneSink, JpegUniform>),
                           dim3((unsigned)((G.mw + per - 1) / per), (unsigned)G.mh, (unsigned)n), dim3(JLay<JL444>::T), 0, st, s, sink, G.mw,
                           G.bw, q, JpegUniform{});
    }
    IMGXF_CHECK(launch_status());
    return imgxf_jpeg_decode_color(planes, images, im.data(), n, d.p, stream);
}

static int rt_list(const void* block_host, const void* block_dev, const imgxf_jpeg_tables* tables, uint8_t* out, size_t out_bytes,
                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!block_host || !tables) return IMGXF_ERR_NULL;
    const u8* hb = (const u8*)block_host;
    imgxf_jpeg_roundtrip_list_header hd;
    memcpy(&hd, hb, sizeof(hd));
    const int n = hd.n_frames;
    if (n < 0 || n > 65535) return IMGXF_ERR_SHAPE;
    if (hd.frames_off != (int32_t)sizeof(hd) ||
        (int64_t)hd.total_bytes < (int64_t)hd.frames_off + (int64_t)n * (int64_t)(sizeof(imgxf_jpeg_list_frame) + sizeof(imgxf_jpeg_dec_image)))
        return IMGXF_ERR_ARG;
    if (n == 0) return IMGXF_OK;
    // the records bound every address the kernels form: the frames' own fields are checked, then the whole block against
    // the one the layout function writes for these sizes
    std::vector<int32_t> sizes;
    std::vector<u8> ref;
    imgxf_jpeg_roundtrip_list_header rhd;
    try {
        sizes.resize((size_t)n * 2);
        for (int i = 0; i < n; ++i) {
            imgxf_jpeg_list_frame f;
            memcpy(&f, hb + hd.frames_off + (size_t)i * sizeof(f), sizeof(f));
            if (!f.data) return IMGXF_ERR_NULL;
            if (f.h < 1 || f.w < 1 || f.h > 32767 || f.w > 32767 || f.row_stride < (int64_t)f.w * 3) return IMGXF_ERR_SHAPE;
            sizes[(size_t)2 * i] = f.h;
            sizes[(size_t)2 * i + 1] = f.w;
        }
        ref.resize((size_t)hd.total_bytes);
        const int rc = rt_list_build(n, sizes.data(), ref.data(), ref.size(), &rhd);
        if (rc == IMGXF_ERR_WORKSPACE) return IMGXF_ERR_ARG;                  // a block of another size is not this layout
        IMGXF_CHECK(rc);
    } catch (const std::bad_alloc&) {
        return IMGXF_ERR_WORKSPACE;
    }
    if (memcmp(&rhd, &hd, sizeof(hd)) != 0) return IMGXF_ERR_ARG;
    constexpr size_t given = offsetof(imgxf_jpeg_list_frame, h);            // data, row_stride: the caller's
    for (int i = 0; i < n; ++i) {
        const size_t o = (size_t)hd.frames_off + (size_t)i * sizeof(imgxf_jpeg_list_frame) + given;
        if (memcmp(ref.data() + o, hb + o, sizeof(imgxf_jpeg_list_frame) - given) != 0) return IMGXF_ERR_ARG;
    }
    const size_t rest = (size_t)hd.images_off;
    if (memcmp(ref.data() + rest, hb + rest, (size_t)hd.total_bytes - rest) != 0) return IMGXF_ERR_ARG;
    if (!block_dev || !out) return IMGXF_ERR_NULL;
    if (((uintptr_t)block_dev) & 7) return IMGXF_ERR_ARG;
    if (!workspace || workspace_bytes < hd.workspace_bytes || (((uintptr_t)workspace) & 15)) return IMGXF_ERR_WORKSPACE;
    if (out_bytes < hd.out_bytes || (((uintptr_t)out) & 15)) return IMGXF_ERR_WORKSPACE;
    JpegQuant q;
    IMGXF_CHECK(jpeg_prepare_quant(q, tables, 3));
    const u8* db = (const u8*)block_dev;
    const imgxf_jpeg_dec_image* images = (const imgxf_jpeg_dec_image*)(db + hd.images_off);
    const JpegList wh = {(const imgxf_jpeg_list_frame*)(db + hd.frames_off), (const imgxf_jpeg_list_unit*)(db + hd.units_off), 0, 0};
    hipLaunchKernelGGL((jpeg_transform_kernel<JpegList, JpegPlaneSink>), dim3((unsigned)hd.n_units), dim3(JT), 0, (hipStream_t)stream, View{},
                       JpegPlaneSink{(u8*)workspace, images}, 0, 0, 0, q, wh);
    IMGXF_CHECK(launch_status());
    // (ref holds the same records as the caller's block, at an address aligned for them)
    return imgxf_jpeg_decode_color((const u8*)workspace, images, (const imgxf_jpeg_dec_image*)(ref.data() + hd.images_off), n, out, stream);
}
