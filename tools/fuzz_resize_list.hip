// Stand-alone CPU program for the HOST code of resize_list.resize_list (csrc/resize_list.hip): lays out blocks for seeded
// random lists — sides 1..32767, all five filters, boxes, frames shared by several entries, budgets from a few bytes to
// 64 KiB — and asserts on every block that the units of an entry tile its oh x ow exactly once (each output pixel in one
// unit), that x0 and every chunk width but the last are multiples of 4, that every unit's LDS, recomputed from the tables
// it reads, stays within its own statement, the header's and the budget, and that the launcher's own record checks accept
// it; hostile geometry must be refused by the layout; mutated and truncated blocks go through the launcher's checks.
// Meant for a sanitizer build of the host side; it never touches a device:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Iimagetransformations_amd/csrc tools/fuzz_resize_list.hip -o _exp/fuzz_resize_list
//     ASAN_OPTIONS=detect_leaks=0 _exp/fuzz_resize_list [rounds] [seed]
// Exit status 0: every block tiled its entries and kept its LDS, every valid block passed, every hostile geometry was
// refused, no mutated block made the checks read outside the block (the sanitizer aborts otherwise).
// The last line printed is a running hash of every return code seen (layouts, launcher, checks of the valid and of the
// mutated blocks): equal seeds and rounds give equal lines for as long as the host code decides the same.
#include "../imagetransformations_amd/csrc/resize_list.hip"
#include <random>
#include <vector>

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 300;
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1u);
    auto uni = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };
    const int filters[] = {IMGXF_RESAMPLE_BILINEAR, IMGXF_RESAMPLE_BICUBIC, IMGXF_RESAMPLE_BOX, IMGXF_RESAMPLE_HAMMING,
                           IMGXF_RESAMPLE_LANCZOS};
    long laid = 0, too_large = 0, entries = 0, beyond = 0, rows_first = 0, chunked = 0, n_units = 0, hostile = 0, refused = 0,
         mutated = 0, rejected = 0;
    uint64_t codes = 1469598103934665603ull;                  // FNV-1a over every return code seen, in order
    auto seen = [&](int rc) { codes = (codes ^ (uint32_t)rc) * 1099511628211ull; return rc; };
    for (int round = 0; round < rounds; ++round) {
        const int n = uni(0, 3) ? uni(0, 24) : uni(0, 200);
        const int budget = uni(0, 2) == 0 ? 65536 : uni(0, 1) ? uni(1, 70000) : uni(1, 4096);
        const int cap = budget < 65536 ? budget : 65536;
        const int filter = filters[uni(0, 4)];
        auto side = [&](int kind) { return kind == 0 ? uni(1, 9) : kind == 1 ? uni(1, 300) : kind == 2 ? uni(1, 3000) : uni(1, 32767); };
        const int n_frames = n ? uni(1, n) : 0;
        std::vector<int> fh(n_frames), fw(n_frames);
        for (int f = 0; f < n_frames; ++f) {
            const int kind = n > 24 ? uni(0, 1) : uni(0, 9) ? uni(0, 2) : 3;
            fh[f] = side(kind); fw[f] = side(uni(0, 4) ? kind : uni(0, 3) % 3);
        }
        std::vector<int32_t> geo((size_t)n * 8 + 1);             // (+ a spare word: an empty list still has an address)
        for (int i = 0; i < n; ++i) {
            int32_t* g = &geo[(size_t)i * 8];
            const int f = uni(0, n_frames - 1);                  // several entries may read one frame
            g[0] = fh[f]; g[1] = fw[f];
            if (uni(0, 1)) { g[2] = g[3] = 0; g[4] = g[0]; g[5] = g[1]; }
            else { g[4] = uni(1, g[0]); g[5] = uni(1, g[1]); g[2] = uni(0, g[0] - g[4]); g[3] = uni(0, g[1] - g[5]); }
            const int okind = n > 24 ? uni(0, 1) : uni(0, 19) ? uni(0, 2) : 3;
            g[6] = uni(0, 5) ? side(okind) : g[4];               // an axis that keeps its length now and then
            g[7] = uni(0, 5) ? side(uni(0, 3) ? okind : uni(0, 2)) : g[5];
        }
        size_t need = 0, need2 = 0;
        int rc = seen(imgxf_resize_list_layout_host(geo.data(), n, filter, budget, nullptr, 0, &need));
        if (rc == IMGXF_ERR_SHAPE || (rc == IMGXF_OK && need > ((size_t)96 << 20))) { ++too_large; continue; }
        if (rc != IMGXF_OK) { fprintf(stderr, "size pass: %d\n", rc); return 2; }
        std::vector<u8> block(need);                              // exactly the stated size: one byte past it is the sanitizer's
        rc = seen(imgxf_resize_list_layout_host(geo.data(), n, filter, budget, block.data(), block.size(), &need2));
        if (rc != IMGXF_OK || need2 != need) { fprintf(stderr, "layout: %d (%zu, %zu)\n", rc, need, need2); return 2; }
        if (seen(imgxf_resize_list_layout_host(geo.data(), n, filter, budget, block.data(), need - 1, &need2)) != IMGXF_ERR_WORKSPACE) {
            fprintf(stderr, "a short block was not refused\n");
            return 2;
        }
        ++laid;
        imgxf_resize_list_header* hd = (imgxf_resize_list_header*)block.data();
        imgxf_resize_list_entry* ent = (imgxf_resize_list_entry*)(block.data() + hd->entries_off);
        const imgxf_resize_list_unit* units = (const imgxf_resize_list_unit*)(block.data() + hd->units_off);
        const int32_t* words = (const int32_t*)block.data();
        for (int i = 0; i < n; ++i) {                             // what the caller fills in
            ent[i].data = 4096; ent[i].row_stride = (int64_t)ent[i].w * 3 + (uni(0, 1) ? 0 : uni(0, 40));
            const bool first = imgxf::rsl_rows_first(ent[i].bh, ent[i].bw, ent[i].oh);
            rows_first += first; beyond += ent[i].unit_rows == 0 && !first; chunked += ent[i].unit_rows && ent[i].chunk < ent[i].ow;
            if (first && ent[i].unit_rows) { fprintf(stderr, "a rows-first entry was taken\n"); return 2; }
        }
        entries += n; n_units += hd->n_units;
        if (hd->lds_bytes > cap) { fprintf(stderr, "LDS %d above the budget %d\n", hd->lds_bytes, budget); return 2; }
        // every output pixel in exactly one unit: the units of an entry come chunk by chunk, band by band, and tile it
        int k = 0;
        for (int i = 0; i < n; ++i) {
            const imgxf_resize_list_entry& e = ent[i];
            if (!e.unit_rows) continue;
            int cx = 0, cy = 0;
            int64_t area = 0;
            for (; k < hd->n_units && units[k].entry == i; ++k) {
                const imgxf_resize_list_unit& u = units[k];
                if (u.x0 != cx || u.y0 != cy || u.ny < 1 || u.nx < 1 || u.y0 + u.ny > e.oh || u.x0 + u.nx > e.ow || (u.x0 & 3) ||
                    ((u.nx & 3) && u.x0 + u.nx != e.ow) || (cx + u.nx < e.ow && u.nx != e.chunk)) {
                    fprintf(stderr, "units do not tile entry %d (round %d)\n", i, round);
                    return 2;
                }
                int c_lo, c_hi, r_lo, r_hi;
                pl_span(words + e.bounds_x, u.x0, u.nx, &c_lo, &c_hi);
                pl_span(words + e.bounds_y, u.y0, u.ny, &r_lo, &r_hi);
                if (c_lo < u.col0 || c_hi > u.col0 + u.ncols || u.col0 < 0 || u.col0 + u.ncols > e.bw || r_lo < 0 || r_hi > e.bh ||
                    pl_lds_bytes(r_hi - r_lo, u.nx, u.ncols) > u.lds_bytes || u.lds_bytes > hd->lds_bytes) {
                    fprintf(stderr, "a unit's LDS or span (entry %d, round %d)\n", i, round);
                    return 2;
                }
                area += (int64_t)u.ny * u.nx;
                cy += u.ny;
                if (cy == e.oh) { cy = 0; cx += u.nx; }
            }
            if (cx != e.ow || cy != 0 || area != (int64_t)e.oh * e.ow) { fprintf(stderr, "entry %d is not covered (round %d)\n", i, round); return 2; }
        }
        if (k != hd->n_units) { fprintf(stderr, "units out of order (round %d)\n", round); return 2; }
        rc = seen(imgxf::resize_list_check(block.data(), block.size(), (size_t)hd->out_bytes));
        if (rc != IMGXF_OK) { fprintf(stderr, "a valid block was rejected: %d (round %d)\n", rc, round); return 2; }
        // the launcher with a valid block and no device block: it must stop at its own NULL check, before any launch
        rc = seen(imgxf_resize_list_u8(block.data(), block.size(), nullptr, nullptr, (size_t)hd->out_bytes, nullptr));
        if (rc != (hd->n_units ? IMGXF_ERR_NULL : IMGXF_OK)) { fprintf(stderr, "launcher: %d\n", rc); return 2; }

        for (int m = 0; m < 40 && n; ++m) {                       // hostile geometry: every one must be refused by the layout
            std::vector<int32_t> bad = geo;
            int32_t* g = &bad[(size_t)uni(0, n - 1) * 8];
            switch (uni(0, 6)) {
                case 0: g[2] = g[0] - g[4] + uni(1, 5); break;               // the box past the bottom
                case 1: g[3] = g[1] - g[5] + uni(1, 5); break;               // past the right edge
                case 2: g[uni(2, 3)] = -uni(1, 9); break;
                case 3: g[uni(4, 5)] = -uni(0, 9); break;                    // empty or negative extent
                case 4: g[uni(2, 5)] = uni(0, 1) ? INT32_MAX : INT32_MIN; break;
                case 5: g[uni(0, 1)] = uni(0, 1) ? 0 : 32768 + uni(0, 9); break;
                default: g[uni(6, 7)] = uni(0, 2) == 0 ? 0 : uni(0, 1) ? 32768 + uni(0, 9) : -uni(1, 9); break;
            }
            ++hostile;
            refused += seen(imgxf_resize_list_layout_host(bad.data(), n, filter, budget, nullptr, 0, &need2)) == IMGXF_ERR_ARG;
        }
        hostile += 2;                                             // a filter that is none of Resample.c's, no budget
        refused += seen(imgxf_resize_list_layout_host(geo.data(), n, uni(0, 1) ? 0 : uni(6, 99), budget, nullptr, 0, &need2)) == IMGXF_ERR_ARG;
        refused += seen(imgxf_resize_list_layout_host(geo.data(), n, filter, -uni(0, 9), nullptr, 0, &need2)) == IMGXF_ERR_ARG;

        const std::vector<u8> good = block;
        const size_t out_bytes = (size_t)hd->out_bytes;
        const size_t records = (size_t)hd->tables_off;            // mutations aim at the header, the records and the units
        for (int m = 0; m < 200; ++m) {                           // mutated blocks through the launcher's checks
            block = good;
            size_t bytes = block.size();
            const int kind = uni(0, 6);
            const int v[] = {0, -1, 1, 3, 4, 15, 16, 17, 1 << 30, INT32_MIN, INT32_MAX, uni(-5, 70000), 32767, 32768};
            if (kind == 0) {                                      // a header word
                ((int32_t*)block.data())[uni(0, 9)] = uni(0, 1) ? uni(-2, 1 << 30) : uni(-2, 600);
            } else if (kind <= 3 && records > sizeof(imgxf_resize_list_header)) {    // a 32-bit field of the records and units
                int32_t* wd = (int32_t*)(block.data() + sizeof(imgxf_resize_list_header));
                wd[uni(0, (int)((records - sizeof(imgxf_resize_list_header)) / 4) - 1)] = v[uni(0, 13)];
            } else if (kind == 4 && need > records + 4) {         // a word of the tables
                int32_t* wd = (int32_t*)(block.data() + records);
                wd[uni(0, (int)((need - records) / 4) - 1)] = v[uni(0, 13)];
            } else if (kind == 5) {                               // a truncated block
                bytes = (size_t)uni(0, (int)bytes);
                block.resize(bytes);
                block.shrink_to_fit();
            } else {                                              // more entries or units than the block holds
                imgxf_resize_list_header* h2 = (imgxf_resize_list_header*)block.data();
                (uni(0, 1) ? h2->n_units : h2->n_entries) += uni(1, 1 << 20);
            }
            ++mutated;
            rejected += seen(imgxf::resize_list_check(block.data(), bytes, uni(0, 3) ? out_bytes : (size_t)uni(0, 4096))) != IMGXF_OK;
        }
    }
    printf("%ld layouts (%ld skipped as too large), %ld entries (%ld beyond the budget, %ld rows first, %ld cut into chunks), "
           "%ld units tiled, %ld of %ld hostile geometries refused, %ld of %ld mutated blocks rejected\n", laid, too_large, entries,
           beyond, rows_first, chunked, n_units, refused, hostile, rejected, mutated);
    printf("return codes: %016llx\n", (unsigned long long)codes);
    return refused == hostile ? 0 : 3;
}
