// Stand-alone CPU program for the HOST code of transform_list.transform_list (csrc/transform_list.hip): lays out blocks for
// seeded random lists — sides 1..32767, both methods, the three filters, coefficients from identities to keystones whose
// horizon lies just outside the output, huge and tiny magnitudes — and asserts on every block that the units of an entry
// tile its oh x ow exactly once on the tile grid, that they are sorted by route as the header states, that a record holds
// its caller's numbers, that a served PERSPECTIVE entry has a denominator strictly of one sign at EVERY pixel centre of its
// first and last rows and columns, and that the launcher's own record checks accept the block; hostile geometry, methods,
// filters and coefficients must be refused by the layout with the code include/imgxf.h states; mutated and truncated
// blocks go through the launcher's checks, up to the point where the launcher would launch (no device block is ever
// given).
// Meant for a sanitizer build of the host side; it never touches a device:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Iimagetransformations_amd/csrc tools/fuzz_transform_list.hip -o _exp/fuzz_transform_list
//     ASAN_OPTIONS=detect_leaks=0 _exp/fuzz_transform_list [rounds] [seed]
// Exit status 0: every block tiled its entries, every valid block passed, every hostile input was refused, no mutated
// block made the checks read outside the block (the sanitizer aborts otherwise).
// The last line printed is a running hash of every return code seen: equal seeds and rounds give equal lines for as long
// as the host code decides the same.
#include "../imagetransformations_amd/csrc/transform_list.hip"
#include <limits>
#include <random>
#include <vector>

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 300;
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1u);
    auto uni = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };
    auto real = [&](double lo, double hi) { return lo + (hi - lo) * (double)(rng() >> 5) / (double)(1u << 27); };
    long laid = 0, too_large = 0, entries = 0, n_units = 0, per_route[6] = {0, 0, 0, 0, 0, 0}, horizons = 0, hostile = 0, refused = 0,
         mutated = 0, rejected = 0, edge_pixels = 0;
    uint64_t codes = 1469598103934665603ull;                  // FNV-1a over every return code seen, in order
    auto seen = [&](int rc) { codes = (codes ^ (uint32_t)rc) * 1099511628211ull; return rc; };
    for (int round = 0; round < rounds; ++round) {
        const int n = uni(0, 3) ? uni(0, 24) : uni(0, 200);
        auto side = [&](int kind) { return kind == 0 ? uni(1, 9) : kind == 1 ? uni(1, 300) : kind == 2 ? uni(1, 3000) : uni(1, 32767); };
        std::vector<int32_t> geo((size_t)n * 4 + 1), meth((size_t)n + 1), filt((size_t)n + 1);   // (+ a spare: an empty list still has an address)
        std::vector<double> co((size_t)n * 8 + 1);
        std::vector<uint8_t> fill((size_t)n * 3 + 1);
        for (int i = 0; i < n; ++i) {
            int32_t* g = &geo[(size_t)i * 4];
            const int kind = n > 24 ? uni(0, 1) : uni(0, 9) ? uni(0, 2) : 3;
            g[0] = side(kind); g[1] = side(uni(0, 4) ? kind : uni(0, 2));
            g[2] = uni(0, 3) ? side(kind) : g[0]; g[3] = uni(0, 3) ? side(uni(0, 3) ? kind : uni(0, 2)) : g[1];
            meth[i] = uni(0, 1); filt[i] = uni(0, 2);
            double* a = &co[(size_t)i * 8];
            const int shape = uni(0, 7);
            for (int k = 0; k < 8; ++k)
                a[k] = shape == 0 ? (k == 0 || k == 4 ? 1.0 : 0.0) : shape == 1 ? real(-1e290, 1e290) : shape == 2 ? real(-1e-300, 1e-300)
                                                                                                              : real(-2.0, 2.0);
            if (meth[i] == IMGXF_TRANSFORM_PERSPECTIVE && shape >= 3) {
                // a horizon at a chosen distance outside (or, one time in four, inside) the output: a6 xin + a7 yin = -1 on it
                const double reach = shape == 3 ? real(1.0, 1.000001) : shape == 4 ? real(0.2, 0.999999) : real(1.0, 50.0);
                const double gx = real(0.0, 1.0), gy = 1.0 - gx, sgn = uni(0, 1) ? 1.0 : -1.0;
                a[6] = sgn * gx / (reach * g[3]); a[7] = sgn * gy / (reach * g[2]);
                if (shape == 7) { a[6] *= -real(1.0, 30.0); a[7] *= -real(1.0, 30.0); }        // strictly negative denominators too
            }
            for (int k = 0; k < 3; ++k) fill[(size_t)i * 3 + k] = (uint8_t)uni(0, 255);
        }
        size_t need = 0, need2 = 0;
        auto lay = [&](void* block, size_t cap, size_t* bytes) {
            return seen(imgxf_transform_list_layout_host(geo.data(), meth.data(), co.data(), filt.data(), fill.data(), n, block, cap, bytes));
        };
        int rc = lay(nullptr, 0, &need);
        if (rc == IMGXF_ERR_UNSUPPORTED) {                        // some PERSPECTIVE entry's horizon crosses its output: it must be one that does
            bool any = false;
            for (int i = 0; i < n; ++i) {
                const bool bad = imgxf::tfl_coeffs_status(meth[i], &co[(size_t)i * 8], geo[(size_t)i * 4 + 2], geo[(size_t)i * 4 + 3]) != IMGXF_OK;
                any |= bad;
                if (bad) {                                        // the same entry as a QUAD is laid out
                    if (meth[i] != IMGXF_TRANSFORM_PERSPECTIVE) { fprintf(stderr, "a QUAD entry was refused (round %d)\n", round); return 2; }
                    meth[i] = IMGXF_TRANSFORM_QUAD;
                }
            }
            if (!any) { fprintf(stderr, "refused without a cause (round %d)\n", round); return 2; }
            ++horizons;
            rc = lay(nullptr, 0, &need);
        }
        if (rc == IMGXF_ERR_SHAPE || (rc == IMGXF_OK && need > ((size_t)96 << 20))) { ++too_large; continue; }
        if (rc != IMGXF_OK) { fprintf(stderr, "size pass: %d\n", rc); return 2; }
        std::vector<u8> block(need);                              // exactly the stated size: one byte past it is the sanitizer's
        rc = lay(block.data(), block.size(), &need2);
        if (rc != IMGXF_OK || need2 != need) { fprintf(stderr, "layout: %d (%zu, %zu)\n", rc, need, need2); return 2; }
        if (lay(block.data(), need - 1, &need2) != IMGXF_ERR_WORKSPACE) { fprintf(stderr, "a short block was not refused\n"); return 2; }
        ++laid;
        imgxf_transform_list_header* hd = (imgxf_transform_list_header*)block.data();
        imgxf_transform_list_entry* ent = (imgxf_transform_list_entry*)(block.data() + hd->entries_off);
        const imgxf_transform_list_unit* units = (const imgxf_transform_list_unit*)(block.data() + hd->units_off);
        entries += n; n_units += hd->n_units;
        std::vector<size_t> next(6);
        for (int r = 0; r < 6; ++r) { next[r] = (size_t)hd->route_first[r]; per_route[r] += hd->route_count[r]; }
        if ((size_t)hd->tables_off != (size_t)hd->units_off + (size_t)hd->n_units * sizeof(imgxf_transform_list_unit) ||
            (size_t)hd->total_bytes != need) { fprintf(stderr, "sections (round %d)\n", round); return 2; }
        for (int i = 0; i < n; ++i) {
            imgxf_transform_list_entry& e = ent[i];
            e.data = 4096; e.row_stride = (int64_t)e.w * 3 + (uni(0, 1) ? 0 : uni(0, 40));     // what the caller fills in
            const double* a = &co[(size_t)i * 8];
            if (e.route != 3 * meth[i] + filt[i] || memcmp(a, e.a, sizeof e.a) || (e.out_off & 15) || memcmp(e.fill, &fill[(size_t)i * 3], 3) ||
                e.h != geo[(size_t)i * 4] || e.w != geo[(size_t)i * 4 + 1] || e.oh != geo[(size_t)i * 4 + 2] || e.ow != geo[(size_t)i * 4 + 3]) {
                fprintf(stderr, "record %d (round %d)\n", i, round);
                return 2;
            }
            // the entry's units come in a row within its route's range, row-major on the tile grid: every pixel once
            for (int y0 = 0; y0 < e.oh; y0 += IMGXF_TRANSFORM_LIST_TILE_H)
                for (int x0 = 0; x0 < e.ow; x0 += IMGXF_TRANSFORM_LIST_TILE_W) {
                    const size_t k = next[e.route]++;
                    if (k >= (size_t)hd->route_first[e.route] + hd->route_count[e.route] || units[k].entry != i || units[k].x0 != x0 ||
                        units[k].y0 != y0) {
                        fprintf(stderr, "units do not tile entry %d (round %d)\n", i, round);
                        return 2;
                    }
                }
            if (meth[i] == IMGXF_TRANSFORM_PERSPECTIVE) {         // what the corner rule promises, on the pixels of the output's edges
                const double s = imgxf::tfl_den(a, 0.5, 0.5);
                auto same = [&](double d) { return s > 0.0 ? d > 0.0 : d < 0.0; };
                bool ok = s != 0.0;
                for (int x = 0; x < e.ow && ok; ++x) ok = same(imgxf::tfl_den(a, x + 0.5, 0.5)) && same(imgxf::tfl_den(a, x + 0.5, e.oh - 0.5));
                for (int y = 0; y < e.oh && ok; ++y) ok = same(imgxf::tfl_den(a, 0.5, y + 0.5)) && same(imgxf::tfl_den(a, e.ow - 0.5, y + 0.5));
                edge_pixels += 2 * ((long)e.ow + e.oh);
                if (!ok) { fprintf(stderr, "a served denominator changes sign on the edge of entry %d (round %d)\n", i, round); return 2; }
            }
        }
        for (int r = 0; r < 6; ++r)
            if (next[r] != (size_t)hd->route_first[r] + hd->route_count[r]) { fprintf(stderr, "route %d's units (round %d)\n", r, round); return 2; }
        rc = seen(imgxf::transform_list_check(block.data(), block.size(), (size_t)hd->out_bytes));
        if (rc != IMGXF_OK) { fprintf(stderr, "a valid block was rejected: %d (round %d)\n", rc, round); return 2; }
        // the launcher with a valid block and no device block: it must stop at its own NULL check, before any launch
        rc = seen(imgxf_transform_list_u8(block.data(), block.size(), nullptr, nullptr, (size_t)hd->out_bytes, nullptr));
        int launches = -1;
        imgxf_transform_list_last_launches(&launches);
        if (rc != (hd->n_units ? IMGXF_ERR_NULL : IMGXF_OK) || launches != 0) { fprintf(stderr, "launcher: %d, %d launches\n", rc, launches); return 2; }

        for (int t = 0; t < 40 && n; ++t) {                       // hostile input: every one must be refused by the layout, with its code
            std::vector<int32_t> bg = geo, bm = meth, bf = filt;
            std::vector<double> bc = co;
            const int i = uni(0, n - 1);
            int want = IMGXF_ERR_ARG;
            switch (uni(0, 5)) {
                case 0: bg[(size_t)i * 4 + uni(0, 3)] = uni(0, 2) == 0 ? 0 : uni(0, 1) ? 32768 + uni(0, 9) : -uni(1, 9); break;
                case 1: bg[(size_t)i * 4 + uni(0, 3)] = uni(0, 1) ? INT32_MAX : INT32_MIN; break;
                case 2: bf[i] = uni(0, 1) ? uni(3, 99) : -uni(1, 9); break;
                case 3: bm[i] = uni(0, 1) ? uni(2, 99) : -uni(1, 9); break;
                case 4: bc[(size_t)i * 8 + uni(0, 7)] = uni(0, 2) == 0 ? std::numeric_limits<double>::quiet_NaN()
                                                        : (uni(0, 1) ? 1 : -1) * std::numeric_limits<double>::infinity(); break;
                default:                                          // above the bound; or a horizon through the output's centre
                    want = IMGXF_ERR_UNSUPPORTED;
                    if (uni(0, 1)) bc[(size_t)i * 8 + uni(0, 7)] = (uni(0, 1) ? 1 : -1) * 1.0000001e290 * pow(10.0, real(0.0, 18.0));
                    else { bm[i] = IMGXF_TRANSFORM_PERSPECTIVE; bc[(size_t)i * 8 + 6] = -2.0 / bg[(size_t)i * 4 + 3]; bc[(size_t)i * 8 + 7] = 0.0;
                           if (bg[(size_t)i * 4 + 3] == 1) bc[(size_t)i * 8 + 6] = -2.0; }     // one column: zero at its centre
                    break;
            }
            ++hostile;
            const int got = seen(imgxf_transform_list_layout_host(bg.data(), bm.data(), bc.data(), bf.data(), fill.data(), n, nullptr, 0, &need2));
            // entries before i may be refused for their own cause first only in `co`, which was laid out: none is
            refused += got == want;
            if (got != want) fprintf(stderr, "hostile input: %d, expected %d (round %d)\n", got, want, round);
        }

        const std::vector<u8> good = block;
        const size_t out_bytes = (size_t)hd->out_bytes;
        for (int t = 0; t < 200; ++t) {                           // mutated blocks through the launcher's checks
            block = good;
            size_t bytes = block.size();
            const int kind = uni(0, 6);
            const int v[] = {0, -1, 1, 3, 4, 15, 16, 17, 1 << 30, INT32_MIN, INT32_MAX, uni(-5, 70000), 32767, 32768};
            if (kind == 0) {                                      // a header word
                ((int32_t*)block.data())[uni(0, 19)] = uni(0, 1) ? uni(-2, 1 << 30) : uni(-2, 600);
            } else if (kind <= 4 && need > sizeof(imgxf_transform_list_header) + 4) {    // a 32-bit word of the records and units
                int32_t* wd = (int32_t*)(block.data() + sizeof(imgxf_transform_list_header));
                wd[uni(0, (int)((need - sizeof(imgxf_transform_list_header)) / 4) - 1)] = v[uni(0, 13)];
            } else if (kind == 5) {                               // a truncated block
                bytes = (size_t)uni(0, (int)bytes);
                block.resize(bytes);
                block.shrink_to_fit();
            } else {                                              // more entries or units than the block holds
                imgxf_transform_list_header* h2 = (imgxf_transform_list_header*)block.data();
                (uni(0, 1) ? h2->n_units : h2->n_entries) += uni(1, 1 << 20);
            }
            ++mutated;
            const size_t ob = uni(0, 3) ? out_bytes : (size_t)uni(0, 4096);
            const int rc2 = seen(imgxf_transform_list_u8(block.data(), bytes, nullptr, nullptr, ob, nullptr));
            imgxf_transform_list_last_launches(&launches);
            if (launches != 0 || rc2 > 0) { fprintf(stderr, "a mutated block reached a launch\n"); return 2; }
            rejected += rc2 != IMGXF_ERR_NULL && rc2 != IMGXF_OK;
        }
    }
    printf("%ld layouts (%ld skipped as too large), %ld entries, %ld units tiled (perspective %ld / %ld / %ld, quad %ld / %ld / %ld by "
           "filter), %ld lists refused for a horizon inside an output, %ld edge pixels of served denominators checked, %ld of %ld "
           "hostile inputs refused with their code, %ld of %ld mutated blocks rejected\n", laid, too_large, entries, n_units, per_route[0],
           per_route[1], per_route[2], per_route[3], per_route[4], per_route[5], horizons, edge_pixels, refused, hostile, rejected, mutated);
    printf("return codes: %016llx\n", (unsigned long long)codes);
    return refused == hostile ? 0 : 3;
}
