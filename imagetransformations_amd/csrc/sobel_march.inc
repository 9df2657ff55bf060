// Sobel, fast path: marching column strips fed by LDS-DMA (same skeleton as
// sepconv_march.inc), exact integer arithmetic.
//   CIN == 3: RGB in -> Pillow L (fixed-point weights) -> 3x3 Sobel -> out   (benchmark configs[2])
//   CIN == 1: L in -> 3x3 Sobel -> out                                        (scipy.ndimage.sobel,
//             /root/reference/transformation.py:339)
// A wavefront owns a strip of 64 lanes x 16 output pixels (16*CIN input bytes per lane and
// row) and marches down a row chunk.  Per row: CIN+1 LDS-DMAs (the strip's bytes + the two
// neighbouring 16-byte blocks for the one-pixel halo), one hand-counted wait + ds_reads,
// L of 18 pixels with two v_dot4_u32_u8 each (19595 = 76*256+139, 38470 = 150*256+70,
// 7471 = 29*256+47), the three newest L rows as packed 16-bit pairs in registers, the stencil
// in packed 16-bit math (v_pk_*_i16), |G|^2 with v_dot2_i32_i16, sqrt in fp32 (exactly
// rounded; agrees with the fp64 definition for every value < 255.5), one 16-byte nt store.
// Borders: SciPy 'reflect' (dcba|abcd|dcba) = replicate the edge pixel for a 3x3 stencil.
#pragma once
#include "sepconv_march.inc"

namespace imgxf {

typedef short i16x2 __attribute__((ext_vector_type(2)));

constexpr int sobel_wave_lds(int CIN, int J) { return J * 1024 * CIN + 1024 + 16 * J + 16; }

__device__ __forceinline__ u32 pk_add16(u32 a, u32 b) { return (u32)__builtin_bit_cast(u32, __builtin_bit_cast(i16x2, a) + __builtin_bit_cast(i16x2, b)); }
__device__ __forceinline__ u32 pk_sub16(u32 a, u32 b) { return (u32)__builtin_bit_cast(u32, __builtin_bit_cast(i16x2, a) - __builtin_bit_cast(i16x2, b)); }
__device__ __forceinline__ u32 pk_shl16(u32 a, int s) { return (u32)__builtin_bit_cast(u32, (i16x2)(__builtin_bit_cast(i16x2, a) << (short)s)); }

template <int CIN, int VARIANT, int J>
__global__ __launch_bounds__(256) void sobel_march_kernel(View src, View dst, int rows_per_wave) {
    constexpr int LB = 16 * CIN;                 // input bytes per lane and row
    constexpr int SB = 1024 * CIN;               // input bytes per strip and row
    constexpr int ND = (CIN + 1);                // DMAs per row: CIN strip blocks + 1 edge block
    extern __shared__ __attribute__((aligned(16))) char sobel_lds[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = blockIdx.y, f = blockIdx.z;
    const int strip = blockIdx.x * (blockDim.x >> 6) + wave;
    const int W = src.w;                          // multiple of 16 (host-checked)
    if (strip * 1024 >= W) return;                // wave-uniform
    const int x0 = strip * 1024 + lane * 16;      // first output pixel of the lane
    const bool active = x0 < W;
    const int xl = active ? x0 : W - 16;          // lanes past the row end re-read the last block
    const bool left_edge = lane == 0, right_edge = active && (lane == 63 || x0 + 16 >= W);
    const bool img_left = x0 == 0, img_right = active && x0 + 16 >= W;
    const int y_begin = chunk * rows_per_wave, y_end = min(src.h, y_begin + rows_per_wave);
    const u8* sbase = src.p + (int64_t)f * src.fs;

    const bool edge_lane = (left_edge && !img_left) || (right_edge && !img_right);
    const int eoff = left_edge ? xl * CIN - 16 : xl * CIN + LB;     // neighbouring 16-byte block

    char* wl = sobel_lds + wave * sobel_wave_lds(CIN, J);
    char* hl = wl + J * SB;
    const u32 lds_main = (u32)(uintptr_t)(__attribute__((address_space(3))) char*)wl;
    const u32 lds_halo = lds_main + J * SB;
    const u32 a_main = lds_main + lane * LB;
    // halo pixel dwords: left = the 4 bytes that end at the lane's first byte, right = the 4
    // bytes that start after its last byte (strip ends: from the edge blocks)
    const u32 a_left = left_edge ? lds_halo + 12 : a_main - 4;
    const u32 a_right = right_edge ? lds_halo + lane * 16 : a_main + LB;
    const u32 step_l = left_edge ? 16 : SB, step_r = right_edge ? 16 : SB;

    auto issue_row = [&](int yi, int slot) {
        const int gy = yi < 0 ? 0 : (yi >= src.h ? src.h - 1 : yi);          // 'reflect' for a 1-pixel halo
        const u8* rowp = sbase + (int64_t)gy * src.rs;
#pragma unroll
        for (int k = 0; k < CIN; ++k) {
            // DMA k moves bytes [k*1024, (k+1)*1024) of the strip row: lane l supplies 16 of them
            const int boff = strip * SB + k * 1024 + lane * 16;
            const int bclamp = min(boff, W * CIN - 16);
            IMGXF_GLDS16(rowp + bclamp, wl + slot * SB + k * 1024, 0);
        }
        if (edge_lane) IMGXF_GLDS16(rowp + eoff, hl + slot * 16, 0);
    };

    // L of the pixel whose first byte is at byte offset `bo` of the packed dwords w[]
    auto lum = [&](const u32* w, int bo) -> u32 {
        if constexpr (CIN == 1) {
            return (w[bo >> 2] >> (8 * (bo & 3))) & 0xffu;
        } else {
            const u32 px = (bo & 3) == 0 ? w[bo >> 2] : __builtin_amdgcn_alignbyte(w[(bo >> 2) + 1], w[bo >> 2], bo & 3);
            const u32 hi = __builtin_amdgcn_udot4(px, 0x001d964cu, 0u, false);        // (76,150,29,0)
            const u32 lo = __builtin_amdgcn_udot4(px, 0x002f468bu, 0x8000u, false);   // (139,70,47,0) + 0x8000
            return ((hi << 8) + lo) >> 16;
        }
    };

    u32 L[3][9];                                   // 3 newest rows, 18 L values each as 16-bit pairs
    const int y_first = y_begin - 1, y_last = y_end + 1;
#pragma unroll
    for (int j = 0; j < J; ++j) issue_row(min(y_first + j, y_last - 1), j);

    int slot = 0;
    for (int base = y_first; base < y_last; base += 3) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int yi = base + s;
            u32 w[4 * CIN + 2];                    // [left dword][own bytes][right dword]
            {
                const u32 am = a_main + slot * SB, al = a_left + slot * step_l, ar = a_right + slot * step_r;
                u32 lw, rw;
                if constexpr (CIN == 3) {
                    u32x4 q0, q1, q2;
                    asm volatile("s_waitcnt vmcnt(%8)\n\t"
                                 "ds_read_b128 %0, %5\n\t"
                                 "ds_read_b128 %1, %5 offset:16\n\t"
                                 "ds_read_b128 %2, %5 offset:32\n\t"
                                 "ds_read_b32 %3, %6\n\t"
                                 "ds_read_b32 %4, %7\n\t"
                                 "s_waitcnt lgkmcnt(0)"
                                 : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(lw), "=&v"(rw)
                                 : "v"(am), "v"(al), "v"(ar), "n"(ND * (J - 1))
                                 : "memory");
                    w[1] = q0.x; w[2] = q0.y; w[3] = q0.z; w[4] = q0.w;
                    w[5] = q1.x; w[6] = q1.y; w[7] = q1.z; w[8] = q1.w;
                    w[9] = q2.x; w[10] = q2.y; w[11] = q2.z; w[12] = q2.w;
                } else {
                    u32x4 q0;
                    asm volatile("s_waitcnt vmcnt(%6)\n\t"
                                 "ds_read_b128 %0, %3\n\t"
                                 "ds_read_b32 %1, %4\n\t"
                                 "ds_read_b32 %2, %5\n\t"
                                 "s_waitcnt lgkmcnt(0)"
                                 : "=&v"(q0), "=&v"(lw), "=&v"(rw)
                                 : "v"(am), "v"(al), "v"(ar), "n"(ND * (J - 1))
                                 : "memory");
                    w[1] = q0.x; w[2] = q0.y; w[3] = q0.z; w[4] = q0.w;
                }
                w[0] = lw; w[4 * CIN + 1] = rw;
            }
            issue_row(min(yi + J, y_last - 1), slot);
            slot = slot + 1 == J ? 0 : slot + 1;

            // ---- L of pixels -1 .. 16 (byte offset of pixel p inside w[]: 4 + p*CIN)
            u32 lv[18];
#pragma unroll
            for (int p = 0; p < 16; ++p) lv[p + 1] = lum(w, 4 + p * CIN);
            lv[0] = img_left ? lv[1] : lum(w, 4 - CIN);
            lv[17] = img_right ? lv[16] : lum(w, 4 + 16 * CIN);
#pragma unroll
            for (int j = 0; j < 9; ++j) L[s][j] = lv[2 * j] | (lv[2 * j + 1] << 16);

            if (yi - y_first >= 2 && yi < y_last) {
                const u32* r0 = L[(s + 1) % 3];   // row y-1
                const u32* r1 = L[(s + 2) % 3];   // row y
                const u32* r2 = L[s];             // row y+1
                u32 cs[9], rd[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    cs[j] = pk_add16(pk_add16(r0[j], r2[j]), pk_shl16(r1[j], 1));   // vertical [1 2 1]
                    rd[j] = pk_sub16(r2[j], r0[j]);                                  // vertical [-1 0 1]
                }
                u32 q[4] = {0, 0, 0, 0};
#pragma unroll
                for (int j = 1; j <= 8; ++j) {
                    // output pixels e = 2j-1, 2j (x = 2j-2, 2j-1) as a packed pair
                    const u32 gx = pk_sub16(cs[j], cs[j - 1]);
                    const u32 mid = __builtin_amdgcn_alignbit(rd[j], rd[j - 1], 16);
                    const u32 gy = pk_add16(pk_add16(rd[j - 1], rd[j]), pk_shl16(mid, 1));
                    u32 o0, o1;
                    if constexpr (VARIANT == IMGXF_SOBEL_X_WRAP) { o0 = gx & 0xffu; o1 = (gx >> 16) & 0xffu; }
                    else if constexpr (VARIANT == IMGXF_SOBEL_Y_WRAP) { o0 = gy & 0xffu; o1 = (gy >> 16) & 0xffu; }
                    else {
                        const u32 t0 = (gx & 0xffffu) | (gy << 16);          // (gx, gy) of the even pixel
                        const u32 t1 = (gx >> 16) | (gy & 0xffff0000u);      // (gx, gy) of the odd pixel
                        const int m0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, t0), __builtin_bit_cast(i16x2, t0), 0, false);
                        const int m1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, t1), __builtin_bit_cast(i16x2, t1), 0, false);
                        u32 pk = 0;
                        pk = __builtin_amdgcn_cvt_pk_u8_f32(__fsqrt_rn((float)m0), 0, pk);
                        pk = __builtin_amdgcn_cvt_pk_u8_f32(__fsqrt_rn((float)m1), 1, pk);
                        o0 = pk & 0xffu; o1 = (pk >> 8) & 0xffu;
                    }
                    const int e = 2 * (j - 1);     // byte index of the even pixel in the 16-byte output
                    q[e >> 2] |= (o0 << (8 * (e & 3))) | (o1 << (8 * ((e + 1) & 3)));
                }
                if (active) {
                    const u32x4 qv = {q[0], q[1], q[2], q[3]};
                    __builtin_nontemporal_store(qv, (u32x4*)(dst.row(f, yi - 1) + x0));
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- what a Sobel call launches, decided apart from launching it (host only: no HIP call, no look at the environment) ----
// The entry points of conv2d.hip launch from this record and imgxf_sobel_plan_host hands it out, so the tests choose their
// geometries from the rule itself.  Both kernels take the frame from blockIdx.z: a batch runs in launches of at most
// SOBEL_MAX_FRAMES frames, each planned for its own frame count.
constexpr int SOBEL_MARCH_J = 4;                 // rows in flight of sobel_march_kernel
constexpr int SOBEL_MAX_FRAMES = 65535;          // grid.z

struct SobelPlan {
    bool march;                                  // sobel_march_kernel, else sobel_kernel (conv2d.hip)
    int nstrips, spb, rpw, nchunks, nchunks0;    // marching: 1 KiB-pixel strips per row, strips per workgroup, rows per wave,
                                                 // row chunks, and the chunks before the doubling that fills the chip (else 0)
    dim3 grid, block;
    size_t lds;
};

// marching needs >= 2 strips (every row step issues its edge DMA), whole 16-pixel lanes, >= 2 rows, and base address, row
// and frame stride of both views as multiples of 16 (the frame stride of a single frame included)
inline bool sobel_march_eligible(const View& s, const View& d) {
    if (s.w % 16 || s.w <= 1024 || s.h < 2) return false;
    if (((uintptr_t)s.p | (uintptr_t)d.p) & 15) return false;
    if ((s.rs | s.fs | d.rs | d.fs) & 15) return false;
    return true;
}

// s.n <= SOBEL_MAX_FRAMES; cin = 1 (L in) or 3 (RGB in)
inline SobelPlan plan_sobel(const View& s, const View& d, int cin, bool no_march) {
    SobelPlan P = SobelPlan();
    P.march = !no_march && sobel_march_eligible(s, d);
    if (!P.march) {                              // 64 x 16 pixel tiles
        P.grid = dim3((unsigned)((s.w + 63) / 64), (unsigned)((s.h + 15) / 16), (unsigned)s.n);
        P.block = dim3(256);
        return P;
    }
    int64_t nchunks = (s.h + 95) / 96;
    P.nchunks0 = (int)nchunks;
    const int nstrips = (s.w + 1023) / 1024;
    // strips per workgroup: the largest of 4 ... 1 that leaves the fewest idle waves in the last workgroup of a row
    int spb = 4, waste = (nstrips + 3) / 4 * 4 - nstrips;
    for (int c = 3; c >= 1; --c) {
        const int w = (nstrips + c - 1) / c * c - nstrips;
        if (w < waste) { waste = w; spb = c; }
    }
    while (nchunks * ((nstrips + spb - 1) / spb) * s.n < 1024 && (s.h + nchunks - 1) / nchunks > 16) nchunks *= 2;
    const int rpw = (int)((s.h + nchunks - 1) / nchunks);
    nchunks = (s.h + rpw - 1) / rpw;
    P.nstrips = nstrips; P.spb = spb; P.rpw = rpw; P.nchunks = (int)nchunks;
    P.grid = dim3((unsigned)((nstrips + spb - 1) / spb), (unsigned)nchunks, (unsigned)s.n);
    P.block = dim3(64 * spb);
    P.lds = (size_t)spb * sobel_wave_lds(cin, SOBEL_MARCH_J);
    return P;
}

// frames [f0, f0 + n) of a view
inline View sobel_frames(const View& v, int f0, int n) {
    View o = v;
    o.p = v.p + (int64_t)f0 * v.fs;
    o.n = n;
    return o;
}

template <int CIN, int VARIANT>
inline int launch_sobel_march(const View& s, const View& d, const SobelPlan& P, hipStream_t st) {
    constexpr int J = SOBEL_MARCH_J;
    hipLaunchKernelGGL((sobel_march_kernel<CIN, VARIANT, J>), P.grid, P.block, P.lds, st, s, d, P.rpw);   // 64 * spb threads, spb * sobel_wave_lds(CIN, J) bytes
    return launch_status();
}

} // namespace imgxf
