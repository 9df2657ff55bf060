// Stand-alone CPU program for the HOST code of affine_list.affine_list (csrc/affine_list.hip): lays out blocks for seeded
// random lists — sides 1..32767, the three filters, matrices from identities to rotations, deep scales and far shifts,
// frames shared by several entries — and asserts on every block that the units of an entry tile its oh x ow exactly once
// on the tile grid, that they are sorted by route as the header states, that a scale entry's tables are
// ImagingScaleAffine's and its span [xmin, xmax) holds exactly the columns with a source inside the frame, that fx is
// affine_fixed_matrix's, and that the launcher's own record checks accept it; hostile geometry, matrices and filters must
// be refused by the layout; mutated and truncated blocks go through the launcher's checks, up to the point where the
// launcher would launch (no device block is ever given).
// Meant for a sanitizer build of the host side; it never touches a device:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Iimagetransformations_amd/csrc tools/fuzz_affine_list.hip -o _exp/fuzz_affine_list
//     ASAN_OPTIONS=detect_leaks=0 _exp/fuzz_affine_list [rounds] [seed]
// Exit status 0: every block tiled its entries, every valid block passed, every hostile input was refused, no mutated
// block made the checks read outside the block (the sanitizer aborts otherwise).
// The last line printed is a running hash of every return code seen: equal seeds and rounds give equal lines for as long
// as the host code decides the same.
#include "../imagetransformations_amd/csrc/affine_list.hip"
#include <limits>
#include <random>
#include <vector>

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 300;
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1u);
    auto uni = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };
    auto real = [&](double lo, double hi) { return lo + (hi - lo) * (double)(rng() >> 5) / (double)(1u << 27); };
    long laid = 0, too_large = 0, entries = 0, n_units = 0, per_route[4] = {0, 0, 0, 0}, out_of_fixed = 0, hostile = 0, refused = 0,
         mutated = 0, rejected = 0;
    uint64_t codes = 1469598103934665603ull;                  // FNV-1a over every return code seen, in order
    auto seen = [&](int rc) { codes = (codes ^ (uint32_t)rc) * 1099511628211ull; return rc; };
    for (int round = 0; round < rounds; ++round) {
        const int n = uni(0, 3) ? uni(0, 24) : uni(0, 200);
        auto side = [&](int kind) { return kind == 0 ? uni(1, 9) : kind == 1 ? uni(1, 300) : kind == 2 ? uni(1, 3000) : uni(1, 32767); };
        std::vector<int32_t> geo((size_t)n * 4 + 1), filt((size_t)n + 1);          // (+ a spare: an empty list still has an address)
        std::vector<double> mat((size_t)n * 6 + 1);
        std::vector<uint8_t> fill((size_t)n * 3 + 1);
        for (int i = 0; i < n; ++i) {
            int32_t* g = &geo[(size_t)i * 4];
            const int kind = n > 24 ? uni(0, 1) : uni(0, 9) ? uni(0, 2) : 3;
            g[0] = side(kind); g[1] = side(uni(0, 4) ? kind : uni(0, 2));
            g[2] = uni(0, 3) ? side(kind) : g[0]; g[3] = uni(0, 3) ? side(uni(0, 3) ? kind : uni(0, 2)) : g[1];
            filt[i] = uni(0, 2);
            double* m = &mat[(size_t)i * 6];
            const int shape = uni(0, 7);
            const double a = real(-3.2, 3.2), z = shape == 3 ? real(0.01, 40.0) : real(0.5, 2.0);
            if (shape <= 2) {                                     // pure scales and shifts, some far outside, some flipped
                m[0] = (uni(0, 5) ? 1 : -1) * (uni(0, 2) ? z : 1.0); m[1] = 0; m[3] = 0; m[4] = (uni(0, 5) ? 1 : -1) * (uni(0, 2) ? z : 1.0);
                m[2] = shape == 2 ? real(-1e5, 1e5) : real(-20, 20) + (m[0] < 0 ? g[1] : 0);
                m[5] = shape == 2 ? real(-3e9, 3e9) : real(-20, 20) + (m[4] < 0 ? g[0] : 0);
                if (shape == 2 && uni(0, 3) == 0) m[0] = real(-1e7, 1e7);
            } else {                                              // rotations about the centre, zoomed; now and then far away
                const double c = cos(a) / z, s = sin(a) / z, cx = g[1] / 2.0, cy = g[0] / 2.0;
                m[0] = c; m[1] = -s; m[2] = cx - (c * cx - s * cy); m[3] = s; m[4] = c; m[5] = cy - (s * cx + c * cy);
                if (shape == 7) m[uni(0, 1) ? 2 : 5] += real(-40000, 40000);
            }
            for (int k = 0; k < 3; ++k) fill[(size_t)i * 3 + k] = (uint8_t)uni(0, 255);
        }
        size_t need = 0, need2 = 0;
        int rc = seen(imgxf_affine_list_layout_host(geo.data(), mat.data(), filt.data(), fill.data(), n, nullptr, 0, &need));
        if (rc == IMGXF_ERR_UNSUPPORTED) {                        // some NEAREST entry leaves fixed point: it must be one that does
            bool any = false;
            for (int i = 0; i < n; ++i)
                any |= filt[i] == IMGXF_FILTER_NEAREST && (mat[(size_t)i * 6 + 1] != 0 || mat[(size_t)i * 6 + 3] != 0) &&
                       !(imgxf::affine_check_fixed(&mat[(size_t)i * 6], geo[(size_t)i * 4 + 3], geo[(size_t)i * 4 + 2]) &&
                         imgxf::affine_fits_fixed(&mat[(size_t)i * 6]));
            if (!any) { fprintf(stderr, "refused without a cause (round %d)\n", round); return 2; }
            ++out_of_fixed;
            for (int i = 0; i < n; ++i)                           // the same list under BILINEAR is laid out
                if (filt[i] == IMGXF_FILTER_NEAREST && (mat[(size_t)i * 6 + 1] != 0 || mat[(size_t)i * 6 + 3] != 0)) filt[i] = IMGXF_FILTER_BILINEAR;
            rc = seen(imgxf_affine_list_layout_host(geo.data(), mat.data(), filt.data(), fill.data(), n, nullptr, 0, &need));
        }
        if (rc == IMGXF_ERR_SHAPE || (rc == IMGXF_OK && need > ((size_t)96 << 20))) { ++too_large; continue; }
        if (rc != IMGXF_OK) { fprintf(stderr, "size pass: %d\n", rc); return 2; }
        std::vector<u8> block(need);                              // exactly the stated size: one byte past it is the sanitizer's
        rc = seen(imgxf_affine_list_layout_host(geo.data(), mat.data(), filt.data(), fill.data(), n, block.data(), block.size(), &need2));
        if (rc != IMGXF_OK || need2 != need) { fprintf(stderr, "layout: %d (%zu, %zu)\n", rc, need, need2); return 2; }
        if (seen(imgxf_affine_list_layout_host(geo.data(), mat.data(), filt.data(), fill.data(), n, block.data(), need - 1, &need2)) !=
            IMGXF_ERR_WORKSPACE) {
            fprintf(stderr, "a short block was not refused\n");
            return 2;
        }
        ++laid;
        imgxf_affine_list_header* hd = (imgxf_affine_list_header*)block.data();
        imgxf_affine_list_entry* ent = (imgxf_affine_list_entry*)(block.data() + hd->entries_off);
        const imgxf_affine_list_unit* units = (const imgxf_affine_list_unit*)(block.data() + hd->units_off);
        const int32_t* words = (const int32_t*)block.data();
        entries += n; n_units += hd->n_units;
        std::vector<size_t> next(4);
        for (int r = 0; r < 4; ++r) { next[r] = (size_t)hd->route_first[r]; per_route[r] += hd->route_count[r]; }
        for (int i = 0; i < n; ++i) {
            imgxf_affine_list_entry& e = ent[i];
            e.data = 4096; e.row_stride = (int64_t)e.w * 3 + (uni(0, 1) ? 0 : uni(0, 40));     // what the caller fills in
            const double* m = &mat[(size_t)i * 6];
            const int want = filt[i] == IMGXF_FILTER_NEAREST ? (m[1] == 0 && m[3] == 0 ? 0 : 1) : filt[i] == IMGXF_FILTER_BILINEAR ? 2 : 3;
            int fx[6] = {0, 0, 0, 0, 0, 0};
            if (want == 1) affine_fixed_matrix(m, fx);
            if (e.route != want || memcmp(fx, e.fx, sizeof fx) || memcmp(m, e.m, sizeof e.m) || (e.out_off & 15)) {
                fprintf(stderr, "record %d (round %d)\n", i, round);
                return 2;
            }
            // the entry's units come in a row within its route's range, row-major on the tile grid: every pixel once
            for (int y0 = 0; y0 < e.oh; y0 += IMGXF_AFFINE_LIST_TILE_H)
                for (int x0 = 0; x0 < e.ow; x0 += IMGXF_AFFINE_LIST_TILE_W) {
                    const size_t k = next[e.route]++;
                    if (k >= (size_t)hd->route_first[e.route] + hd->route_count[e.route] || units[k].entry != i || units[k].x0 != x0 ||
                        units[k].y0 != y0) {
                        fprintf(stderr, "units do not tile entry %d (round %d)\n", i, round);
                        return 2;
                    }
                }
            if (e.route == IMGXF_AFFINE_LIST_SCALE) {             // ImagingScaleAffine, restated
                double xo = m[2] + m[0] * 0.5, yo = m[5] + m[4] * 0.5;
                int xmin = e.ow, xmax = 0;
                for (int x = 0; x < e.ow; ++x, xo += m[0]) {
                    const int32_t v = xo < 0.0 ? -1 : (xo >= 2147483648.0 ? INT32_MAX : (int32_t)xo);
                    if (v >= 0 && v < e.w) { xmax = x + 1; if (x < xmin) xmin = x; }
                    if (words[e.xtab + x] != v) { fprintf(stderr, "xin of entry %d (round %d)\n", i, round); return 2; }
                }
                for (int y = 0; y < e.oh; ++y, yo += m[4])
                    if (words[e.ytab + y] != (yo < 0.0 ? -1 : (yo >= 2147483648.0 ? INT32_MAX : (int32_t)yo))) {
                        fprintf(stderr, "yin of entry %d (round %d)\n", i, round);
                        return 2;
                    }
                if (xmin != e.xmin || xmax != e.xmax) { fprintf(stderr, "span of entry %d (round %d)\n", i, round); return 2; }
                for (int x = 0; x < e.ow; ++x)                    // the span is exactly the set of columns inside (monotone xo)
                    if ((x >= xmin && x < xmax) != (words[e.xtab + x] >= 0 && words[e.xtab + x] < e.w)) {
                        fprintf(stderr, "a hole in the span of entry %d (round %d)\n", i, round);
                        return 2;
                    }
            }
        }
        for (int r = 0; r < 4; ++r)
            if (next[r] != (size_t)hd->route_first[r] + hd->route_count[r]) { fprintf(stderr, "route %d's units (round %d)\n", r, round); return 2; }
        rc = seen(imgxf::affine_list_check(block.data(), block.size(), (size_t)hd->out_bytes));
        if (rc != IMGXF_OK) { fprintf(stderr, "a valid block was rejected: %d (round %d)\n", rc, round); return 2; }
        // the launcher with a valid block and no device block: it must stop at its own NULL check, before any launch
        rc = seen(imgxf_affine_list_u8(block.data(), block.size(), nullptr, nullptr, (size_t)hd->out_bytes, nullptr));
        int launches = -1;
        imgxf_affine_list_last_launches(&launches);
        if (rc != (hd->n_units ? IMGXF_ERR_NULL : IMGXF_OK) || launches != 0) { fprintf(stderr, "launcher: %d, %d launches\n", rc, launches); return 2; }

        for (int t = 0; t < 40 && n; ++t) {                       // hostile input: every one must be refused by the layout
            std::vector<int32_t> bg = geo, bf = filt;
            std::vector<double> bm = mat;
            const int i = uni(0, n - 1);
            switch (uni(0, 3)) {
                case 0: bg[(size_t)i * 4 + uni(0, 3)] = uni(0, 2) == 0 ? 0 : uni(0, 1) ? 32768 + uni(0, 9) : -uni(1, 9); break;
                case 1: bg[(size_t)i * 4 + uni(0, 3)] = uni(0, 1) ? INT32_MAX : INT32_MIN; break;
                case 2: bf[i] = uni(0, 1) ? uni(3, 99) : -uni(1, 9); break;
                default: bm[(size_t)i * 6 + uni(0, 5)] = uni(0, 2) == 0 ? std::numeric_limits<double>::quiet_NaN()
                                                         : (uni(0, 1) ? 1 : -1) * std::numeric_limits<double>::infinity(); break;
            }
            ++hostile;
            refused += seen(imgxf_affine_list_layout_host(bg.data(), bm.data(), bf.data(), fill.data(), n, nullptr, 0, &need2)) == IMGXF_ERR_ARG;
        }

        const std::vector<u8> good = block;
        const size_t out_bytes = (size_t)hd->out_bytes;
        const size_t records = (size_t)hd->tables_off;            // mutations aim at the header, the records and the units
        for (int t = 0; t < 200; ++t) {                           // mutated blocks through the launcher's checks
            block = good;
            size_t bytes = block.size();
            const int kind = uni(0, 6);
            const int v[] = {0, -1, 1, 3, 4, 15, 16, 17, 1 << 30, INT32_MIN, INT32_MAX, uni(-5, 70000), 32767, 32768};
            if (kind == 0) {                                      // a header word
                ((int32_t*)block.data())[uni(0, 15)] = uni(0, 1) ? uni(-2, 1 << 30) : uni(-2, 600);
            } else if (kind <= 3 && records > sizeof(imgxf_affine_list_header)) {    // a 32-bit field of the records and units
                int32_t* wd = (int32_t*)(block.data() + sizeof(imgxf_affine_list_header));
                wd[uni(0, (int)((records - sizeof(imgxf_affine_list_header)) / 4) - 1)] = v[uni(0, 13)];
            } else if (kind == 4 && need > records + 4) {         // a word of the tables
                int32_t* wd = (int32_t*)(block.data() + records);
                wd[uni(0, (int)((need - records) / 4) - 1)] = v[uni(0, 13)];
            } else if (kind == 5) {                               // a truncated block
                bytes = (size_t)uni(0, (int)bytes);
                block.resize(bytes);
                block.shrink_to_fit();
            } else {                                              // more entries or units than the block holds
                imgxf_affine_list_header* h2 = (imgxf_affine_list_header*)block.data();
                (uni(0, 1) ? h2->n_units : h2->n_entries) += uni(1, 1 << 20);
            }
            ++mutated;
            const size_t ob = uni(0, 3) ? out_bytes : (size_t)uni(0, 4096);
            const int rc2 = seen(imgxf_affine_list_u8(block.data(), bytes, nullptr, nullptr, ob, nullptr));
            imgxf_affine_list_last_launches(&launches);
            if (launches != 0 || rc2 > 0) { fprintf(stderr, "a mutated block reached a launch\n"); return 2; }
            rejected += rc2 != IMGXF_ERR_NULL && rc2 != IMGXF_OK;
        }
    }
    printf("%ld layouts (%ld skipped as too large), %ld entries, %ld units tiled (scale %ld, fixed %ld, bilinear %ld, bicubic %ld), "
           "%ld lists refused for a NEAREST entry outside fixed point, %ld of %ld hostile inputs refused, %ld of %ld mutated blocks "
           "rejected\n", laid, too_large, entries, n_units, per_route[0], per_route[1], per_route[2], per_route[3], out_of_fixed,
           refused, hostile, rejected, mutated);
    printf("return codes: %016llx\n", (unsigned long long)codes);
    return refused == hostile ? 0 : 3;
}
