// Stand-alone CPU program for the HOST code of tensor_maps.resized_crop_list (csrc/resized_crop_list.hip): lays out blocks
// for seeded random and hostile geometry (boxes past their frames, empty and negative extents, sizes at and past the
// limits, tiny budgets) and a filter drawn per round, checks every accepted block with the launcher's own record checks,
// then feeds those checks mutated and truncated blocks.  Before that, a sweep of the kernel's own row builder as the host
// compiles it (rcl_build_row is __host__ __device__: one body) against build_coeffs for BILINEAR, BICUBIC and BOX, every
// (in, out) in 1..130 and a few large sizes: bounds and coefficients equal, every coefficient |k| < 2^23 (what the band
// engine's signed 24-bit multiply holds).  Meant for a sanitizer build of the host side; it never touches a device:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Iimagetransformations_amd/csrc tools/fuzz_resized_crop_list.hip -o _exp/fuzz_resized_crop_list
//     ASAN_OPTIONS=detect_leaks=0 _exp/fuzz_resized_crop_list [rounds] [seed]
// Exit status 0: the row builder equals build_coeffs, every valid block passed, every hostile geometry was refused, no
// mutated block made the checks read outside the block (the sanitizer aborts otherwise).
// The last line printed is a running hash of every return code seen (layouts, launcher, checks of the valid and of the
// mutated blocks): equal seeds and rounds give equal lines for as long as the host code decides the same.
#include "../imagetransformations_amd/csrc/resized_crop_list.hip"
#include <random>
#include <vector>

// rcl_build_row<FILTER> row by row against build_coeffs' tables for (in -> out); HAMMING and LANCZOS tables (host-built
// only) get the range check alone.  Returns the number of rows compared, -1 on a difference.
template <int FILTER>
static long sweep_rows(int in, int out) {
    std::vector<int> bounds, kk;
    const int ks = build_coeffs(in, out, FILTER, bounds, kk);
    if (ks != coeff_ksize(in, out, FILTER)) { fprintf(stderr, "ksize (%d -> %d, filter %d)\n", in, out, FILTER); return -1; }
    for (int v : kk)
        if (v <= -(1 << 23) || v >= (1 << 23)) { fprintf(stderr, "|k| >= 2^23 (%d -> %d, filter %d): %d\n", in, out, FILTER, v); return -1; }
    if constexpr (filter_polynomial(FILTER)) {
        std::vector<int> row((size_t)ks);                     // exactly ksize slots: one tap past them is the sanitizer's
        for (int xx = 0; xx < out; ++xx) {
            int b[2];
            std::fill(row.begin(), row.end(), 0);
            rcl_build_row<FILTER>(in, out, xx, b, row.data());
            if (b[0] != bounds[2 * xx] || b[1] != bounds[2 * xx + 1] || b[1] > ks ||
                memcmp(row.data(), &kk[(size_t)xx * ks], (size_t)ks * 4)) {
                fprintf(stderr, "row builder differs from build_coeffs (%d -> %d, filter %d, row %d)\n", in, out, FILTER, xx);
                return -1;
            }
        }
        return out;
    }
    return 0;
}

static long sweep() {
    std::vector<int> sizes;
    for (int v = 1; v <= 130; ++v) sizes.push_back(v);
    for (int v : {224, 255, 256, 257, 499, 500, 1000, 2240, 4099}) sizes.push_back(v);
    long rows = 0;
    for (int in : sizes)
        for (int out : sizes) {
            const long r[] = {sweep_rows<IMGXF_RESAMPLE_BILINEAR>(in, out), sweep_rows<IMGXF_RESAMPLE_BICUBIC>(in, out),
                              sweep_rows<IMGXF_RESAMPLE_BOX>(in, out), sweep_rows<IMGXF_RESAMPLE_HAMMING>(in, out),
                              sweep_rows<IMGXF_RESAMPLE_LANCZOS>(in, out)};
            for (long v : r) { if (v < 0) return -1; rows += v; }
        }
    return rows;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1u);
    auto uni = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };
    const long swept = sweep();
    if (swept < 0) return 4;
    printf("row builder == build_coeffs on %ld table rows (BILINEAR, BICUBIC, BOX; |k| < 2^23 for all five filters)\n", swept);
    const int filters[] = {IMGXF_RESAMPLE_BILINEAR, IMGXF_RESAMPLE_BICUBIC, IMGXF_RESAMPLE_BOX, IMGXF_RESAMPLE_HAMMING,
                           IMGXF_RESAMPLE_LANCZOS};
    long laid = 0, accepted = 0, hostile = 0, refused = 0, mutated = 0, rejected = 0, entries = 0, beyond = 0, tall = 0;
    uint64_t codes = 1469598103934665603ull;                  // FNV-1a over every return code seen, in order
    auto seen = [&](int rc) { codes = (codes ^ (uint32_t)rc) * 1099511628211ull; return rc; };
    for (int round = 0; round < rounds; ++round) {
        const int n = uni(0, 300);
        const int sh = uni(0, 3) ? uni(1, 300) : uni(1, 5), sw = uni(0, 3) ? uni(1, 300) : uni(1, 5);
        const int budget = uni(0, 3) ? 65536 : uni(1, 70000);
        const int filter = filters[uni(0, 4)];
        const bool built = filter_polynomial(filter);         // the launch builds this filter's tables
        std::vector<int32_t> geo((size_t)n * 7 + 1);             // (+ a spare word: an empty list still has an address)
        for (int i = 0; i < n; ++i) {
            int32_t* g = &geo[(size_t)i * 7];
            const int kind = uni(0, 5);
            g[0] = kind == 0 ? uni(1, 8) : kind == 1 ? uni(1, 32767) : uni(1, 700);
            g[1] = kind == 1 ? uni(1, 8) : kind == 0 ? uni(1, 32767) : uni(1, 700);
            g[4] = uni(1, g[0]); g[5] = uni(1, g[1]);
            g[2] = uni(0, g[0] - g[4]); g[3] = uni(0, g[1] - g[5]);
            g[6] = uni(0, 1);
        }
        size_t need = 0, need2 = 0;
        int rc = seen(imgxf_resized_crop_list_layout_filter_host(geo.data(), n, sh, sw, filter, budget, nullptr, 0, &need));
        if (rc != IMGXF_OK) { fprintf(stderr, "size pass: %d\n", rc); return 2; }
        std::vector<u8> block(need);                          // exactly the stated size: one byte past it is the sanitizer's
        rc = seen(imgxf_resized_crop_list_layout_filter_host(geo.data(), n, sh, sw, filter, budget, block.data(), block.size(), &need2));
        if (rc != IMGXF_OK || need2 != need) { fprintf(stderr, "layout: %d (%zu, %zu)\n", rc, need, need2); return 2; }
        if (need && seen(imgxf_resized_crop_list_layout_filter_host(geo.data(), n, sh, sw, filter, budget, block.data(), need - 1, &need2)) != IMGXF_ERR_WORKSPACE) {
            fprintf(stderr, "a short block was not refused\n");
            return 2;
        }
        ++laid;
        imgxf_resized_crop_header* hd = (imgxf_resized_crop_header*)block.data();
        imgxf_resized_crop_entry* ent = (imgxf_resized_crop_entry*)(block.data() + hd->entries_off);
        for (int i = 0; i < n; ++i) {                         // what the caller fills in
            ent[i].data = 4096; ent[i].row_stride = (int64_t)ent[i].w * 3 + (uni(0, 1) ? 0 : uni(0, 40));
            beyond += ent[i].unit_rows == 0; tall += ent[i].tall;
        }
        entries += n;
        if (hd->lds_bytes > (budget < 65536 ? budget : 65536)) { fprintf(stderr, "LDS %d above the budget %d\n", hd->lds_bytes, budget); return 2; }
        rc = seen(imgxf::resized_crop_list_check(block.data(), block.size(), filter));
        if (rc != IMGXF_OK) { fprintf(stderr, "a valid block was rejected: %d (round %d)\n", rc, round); return 2; }
        ++accepted;
        // the launcher with a valid block and no device block: it must stop at its own NULL check, before any launch
        // (a filter whose tables the kernel does not build is refused before anything else)
        rc = seen(imgxf_resized_crop_list_filter(block.data(), block.size(), nullptr, nullptr, 0, filter, nullptr, nullptr, nullptr));
        if (rc != (!built ? IMGXF_ERR_UNSUPPORTED : hd->n_units ? IMGXF_ERR_NULL : IMGXF_OK)) { fprintf(stderr, "launcher: %d\n", rc); return 2; }
        if (seen(imgxf_resized_crop_list_filter(block.data(), block.size(), nullptr, nullptr, 0, uni(0, 1) ? 0 : 6, nullptr, nullptr, nullptr)) != IMGXF_ERR_ARG) {
            fprintf(stderr, "an unknown filter was not refused\n");
            return 2;
        }

        for (int m = 0; m < 40 && n; ++m) {                   // hostile geometry: every one must be refused by the layout
            std::vector<int32_t> bad = geo;
            int32_t* g = &bad[(size_t)uni(0, n - 1) * 7];
            switch (uni(0, 7)) {
                case 0: g[2] = g[0] - g[4] + uni(1, 5); break;               // the box past the bottom
                case 1: g[3] = g[1] - g[5] + uni(1, 5); break;               // past the right edge
                case 2: g[uni(2, 3)] = -uni(1, 9); break;
                case 3: g[uni(4, 5)] = -uni(0, 9); break;                    // empty or negative extent
                case 4: g[uni(2, 5)] = uni(0, 1) ? INT32_MAX : INT32_MIN; break;
                case 5: g[uni(0, 1)] = uni(0, 1) ? 0 : 32768 + uni(0, 9); break;
                case 6: g[6] = uni(0, 1) ? 2 : -1; break;
                default: g[4] = g[0] + 1; g[2] = 0; break;
            }
            ++hostile;
            refused += seen(imgxf_resized_crop_list_layout_filter_host(bad.data(), n, sh, sw, filter, budget, nullptr, 0, &need2)) == IMGXF_ERR_ARG;
        }
        const int bad_sizes[] = {0, -1, 32768, INT32_MAX, INT32_MIN};
        hostile += 1;                                         // a filter that is none of Resample.c's
        refused += seen(imgxf_resized_crop_list_layout_filter_host(geo.data(), n, sh, sw, uni(0, 1) ? 0 : uni(6, 99), budget, nullptr, 0, &need2)) == IMGXF_ERR_ARG;
        for (int v : bad_sizes) {
            hostile += 2;
            refused += seen(imgxf_resized_crop_list_layout_filter_host(geo.data(), n, v, sw, filter, budget, nullptr, 0, &need2)) == IMGXF_ERR_ARG;
            refused += seen(imgxf_resized_crop_list_layout_filter_host(geo.data(), n, sh, v, filter, budget, nullptr, 0, &need2)) == IMGXF_ERR_ARG;
        }

        const std::vector<u8> good = block;
        for (int m = 0; m < 300; ++m) {                       // mutated blocks through the launcher's checks
            block = good;
            size_t bytes = block.size();
            const int kind = uni(0, 5);
            if (kind == 0) {                                  // a header word
                ((int32_t*)block.data())[uni(0, 7)] = uni(0, 1) ? uni(-2, 1 << 30) : uni(-2, 600);
            } else if (kind <= 3 && need > sizeof(imgxf_resized_crop_header)) {   // a 32-bit field of the records and units
                int32_t* wd = (int32_t*)(block.data() + sizeof(imgxf_resized_crop_header));
                const int nw = (int)((need - sizeof(imgxf_resized_crop_header)) / 4);
                const int v[] = {0, -1, 1, 15, 16, 17, 1 << 30, INT32_MIN, INT32_MAX, uni(-5, 70000), 32767, 32768};
                wd[uni(0, nw - 1)] = v[uni(0, 11)];
            } else if (kind == 4) {                           // a truncated block
                bytes = (size_t)uni(0, (int)bytes);
                block.resize(bytes);
                block.shrink_to_fit();
            } else {                                          // more entries or units than the block holds
                imgxf_resized_crop_header* h2 = (imgxf_resized_crop_header*)block.data();
                (uni(0, 1) ? h2->n_units : h2->n_entries) += uni(1, 1 << 20);
            }
            ++mutated;
            rejected += seen(imgxf::resized_crop_list_check(block.data(), bytes, filter)) != IMGXF_OK;
        }
    }
    printf("%ld layouts (%ld entries, %ld beyond the budget, %ld tall), %ld valid blocks accepted, %ld of %ld hostile geometries "
           "refused, %ld of %ld mutated blocks rejected\n", laid, entries, beyond, tall, accepted, refused, hostile, rejected, mutated);
    printf("return codes: %016llx\n", (unsigned long long)codes);
    return refused == hostile ? 0 : 3;
}
