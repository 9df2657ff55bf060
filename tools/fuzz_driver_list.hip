// Stand-alone CPU program for the HOST code of the list pass (csrc/driver_list.hip with sepconv_route.h): lays out a few
// hundred random entries of every type, blur included, checks the blocks with the device half's own host checks, then
// feeds those checks mutated blocks.  Meant for a sanitizer build of the host side; it never touches a device:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Iimagetransformations_amd/csrc tools/fuzz_driver_list.hip -o _exp/fuzz_driver_list
//     ASAN_OPTIONS=detect_leaks=0 _exp/fuzz_driver_list [rounds] [seed]
// Exit status 0: every valid block passed, no mutated block made the checks read outside the block (the sanitizer aborts
// otherwise).  The last line printed is a running hash of every return code seen (layouts, checks of the valid and of the
// mutated blocks): equal seeds and rounds give equal lines for as long as the host code decides the same.  The two symbols driver_list.hip takes from other translation units are given here.
#include "../imagetransformations_amd/csrc/driver_list.hip"
#include <random>
#include <vector>

namespace imgxf {
const KnobTable& knob_table() {
    static KnobTable t;                                       // no knob set
    return t;
}
int driver_list_blur_launch(bool, int, const u8*, int, int, int, int, u8*, hipStream_t) { return IMGXF_ERR_UNSUPPORTED; }
} // namespace imgxf

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 40;
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1u);
    auto uni = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };
    auto real = [&](double lo, double hi) { return lo + (hi - lo) * (rng() / 4294967296.0); };
    const int types[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 12, 13, 9, 11};
    const int widths[] = {1, 7, 16, 61, 64, 85, 86, 96, 100, 352, 500, 1024};
    long laid = 0, accepted = 0, mutated = 0, rejected = 0, family = 0;
    uint64_t codes = 1469598103934665603ull;                  // FNV-1a over every return code seen, in order
    auto seen = [&](int rc) { codes = (codes ^ (uint32_t)rc) * 1099511628211ull; return rc; };
    for (int round = 0; round < rounds; ++round) {
        const int n = uni(0, 400);
        std::vector<int32_t> geo((size_t)n * 5);
        std::vector<double> par((size_t)n * 2);
        for (int i = 0; i < n; ++i) {
            const int t = types[uni(0, 15)];
            const int h = uni(1, 3) == 1 ? uni(1, 8) : uni(1, 400);
            const int w = uni(0, 1) ? widths[uni(0, 11)] : uni(1, 520);
            int32_t* g = &geo[(size_t)i * 5];
            g[0] = uni(0, 63); g[1] = t; g[2] = h; g[3] = w; g[4] = uni(0, 40) ? 3 : uni(0, 4);
            double p0 = real(-2.0, 2.0), p1 = real(-2.0, 2.0);
            if (t == 0) p0 = real(0.05, 2.5);
            if (t == 1 || t == 5) { p0 = real(-400.0, 400.0); p1 = real(-400.0, 400.0); }
            if (t == 8) { p0 = uni(-1, w); p1 = uni(-1, h); }
            if (t == 12 || t == 13) {
                p0 = uni(0, 12) ? 2 * uni(0, 15) + 1 : uni(-3, 36);
                p1 = uni(0, 9) ? 0.5 * uni(1, 10) : real(-1.0, 8.0);
                if (!uni(0, 60)) p1 = NAN;
                if (!uni(0, 60)) p0 = 3.5;
            }
            par[(size_t)i * 2] = p0; par[(size_t)i * 2 + 1] = p1;
        }
        const int budget = uni(0, 3) ? 65536 : uni(1, 70000);
        size_t need = 0;
        int rc = seen(imgxf_driver_list_layout_host(geo.data(), par.data(), n, budget, nullptr, 0, &need, nullptr, nullptr,
                                                    nullptr, nullptr, nullptr));
        if (rc != IMGXF_OK) { fprintf(stderr, "size pass: %d\n", rc); return 2; }
        std::vector<u8> block(need);                          // exactly the stated size: one byte past it is the sanitizer's
        std::vector<int64_t> off((size_t)n);
        std::vector<int32_t> hw((size_t)n * 2), status((size_t)n);
        size_t need2 = 0, out_bytes = 0;
        int32_t lds = 0;
        rc = seen(imgxf_driver_list_layout_host(geo.data(), par.data(), n, budget, block.data(), block.size(), &need2,
                                                off.data(), hw.data(), status.data(), &out_bytes, &lds));
        if (rc != IMGXF_OK || need2 != need) { fprintf(stderr, "layout: %d (%zu, %zu)\n", rc, need, need2); return 2; }
        ++laid;
        imgxf_driver_header* hd = (imgxf_driver_header*)block.data();
        imgxf_driver_entry* ent = (imgxf_driver_entry*)(block.data() + hd->entries_off);
        imgxf_driver_unit* units = (imgxf_driver_unit*)(block.data() + hd->units_off);
        for (int i = 0; i < n; ++i) {                         // what the caller fills in
            ent[i].src = 4096; ent[i].src_stride = (int64_t)ent[i].w * 3 + (uni(0, 1) ? 0 : uni(0, 40)); ent[i].noise = 8192;
            family += status[i] == IMGXF_DRIVER_REFUSED_FAMILY;
            if (status[i] == IMGXF_DRIVER_REFUSED_FAMILY && (geo[(size_t)i * 5 + 1] != IMGXF_DRIVER_BLUR || geo[(size_t)i * 5 + 3] * 3 % 16)) {
                fprintf(stderr, "REFUSED_FAMILY for type %d, width %d\n", geo[(size_t)i * 5 + 1], geo[(size_t)i * 5 + 3]);
                return 2;
            }
        }
        // every blur unit: a band of its entry, its taps inside the block, runs in ascending (fixed, R)
        for (int k = hd->n_units - hd->n_blur; k < hd->n_units; ++k) {
            const imgxf_driver_entry& e = ent[units[k].entry];
            if (!dl_blurs(e.op) || units[k].y0 + units[k].ny > e.h || units[k].ny > 32 ||
                (size_t)(e.coeffs_x + e.ksx) * 4 > need || e.coeffs_x * 4 < hd->tables_off) {
                fprintf(stderr, "blur unit %d is wrong\n", k);
                return 2;
            }
        }
        rc = seen(driver_list_check(block.data(), (void*)4096, (const uint8_t*)4096, out_bytes));
        if (rc != IMGXF_OK) { fprintf(stderr, "a valid block was rejected: %d (round %d)\n", rc, round); return 2; }
        ++accepted;
        if (!hd->n_units) continue;
        const std::vector<u8> good = block;
        const size_t tables = (size_t)hd->tables_off;
        for (int m = 0; m < 300; ++m) {
            block = good;
            const int kind = uni(0, 5);
            if (kind == 0) {                                  // a header word
                ((int32_t*)block.data())[uni(0, 11)] = uni(0, 1) ? uni(-2, 1 << 30) : uni(-2, 600);
            } else if (kind <= 3) {                           // a 32-bit field of the records and units
                int32_t* wd = (int32_t*)(block.data() + sizeof(imgxf_driver_header));
                const int nw = (int)((tables - sizeof(imgxf_driver_header)) / 4);
                const int v[] = {0, -1, 1, 31, 32, 33, 1 << 30, INT32_MIN, INT32_MAX, uni(-5, 70000), (int)(need / 4), (int)(need / 4) - uni(0, 40)};
                wd[uni(0, nw - 1)] = v[uni(0, 11)];
            } else if (kind == 4 && hd->n_blur) {             // a blur record's own fields
                const imgxf_driver_unit& u = units[hd->n_units - 1 - uni(0, hd->n_blur - 1)];
                imgxf_driver_entry& e = ((imgxf_driver_entry*)(block.data() + hd->entries_off))[u.entry];
                const int which = uni(0, 5);
                const int v = uni(0, 2) ? uni(-3, 40) : (int)(need / 4) - uni(-2, 33);
                (which == 0 ? e.ksx : which == 1 ? e.ksy : which == 2 ? e.coeffs_x : which == 3 ? e.coeffs_y : which == 4 ? e.oh : e.unit_rows) = v;
            } else {                                          // a table word
                if (tables + 4 > need) continue;
                ((int32_t*)(block.data() + tables))[uni(0, (int)((need - tables) / 4) - 1)] = uni(0, 1) ? uni(-40000, 40000) : INT32_MAX;
            }
            ++mutated;
            rejected += seen(driver_list_check(block.data(), (void*)4096, (const uint8_t*)4096, out_bytes)) != IMGXF_OK;
        }
    }
    printf("%ld layouts, %ld valid blocks accepted, %ld of %ld mutated blocks rejected, %ld entries refused for family\n", laid,
           accepted, rejected, mutated, family);
    printf("return codes: %016llx\n", (unsigned long long)codes);
    return 0;
}
