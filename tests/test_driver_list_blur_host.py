"""Host half of driver_list.apply_list for blur entries: codes and statuses, which (size, radius) pairs the per-type
dispatcher serves with the LDS-tiled kernel (taken) and which with another family (refused, float mode only), the blur
units' section, order and bands, the shared tap tables against the oracle, and the device half's checks of the new
records.  No device."""
import numpy as np
import pytest

from oracle import imgxf_oracle as O

RADII = [0.5 * k for k in range(1, 11)]                       # the drivers' grid without radius 0
SIZES = [(40, 352), (40, 96), (24, 96), (37, 61), (334, 500)]  # (h, w); frame index = position
BLUR, BLUR_FIXED = 12, 13


def _dl():
    from imagetransformations_amd import driver_list
    return driver_list


def _ksize(radius):
    from imagetransformations_amd import transformation as T
    return T._blur_ksize(radius)


def _layout(entries, code=BLUR, sizes=SIZES):
    """entries: (frame, radius) blurs, or (frame, type, args) of another type."""
    dl = _dl()
    geo, par = [], []
    for ent in entries:
        f = ent[0]
        if len(ent) == 2:
            geo.append((f, code, sizes[f][0], sizes[f][1], 3))
            par.append((_ksize(ent[1]), ent[1]))
        else:
            geo.append((f, dl.TYPES[ent[1]], sizes[f][0], sizes[f][1], 3))
            par.append(dl.entry_params(ent[1], ent[2]))
    return dl.layout(geo, par)


def expected_status(h, w, radius, fixed=False):
    """What the issue states for the sizes of this file (and of tests/test_gpu_driver_list_blur.py): in float mode rows of
    1056 bytes go to the marching kernel (R <= 4) or the matrix cores (R >= 6), 288-byte rows of 40 lines to the matrix
    cores from R = 6; everything else here is the tile kernel's.  Fixed mode takes them all."""
    dl = _dl()
    if _ksize(radius) == 0:
        return dl.REFUSED_SIZE
    if fixed:
        return dl.OK
    R = _ksize(radius) // 2
    if (h, w) == (40, 352) or ((h, w) == (40, 96) and R >= 6):
        return dl.REFUSED_FAMILY
    return dl.OK


def test_codes_and_parameter_statuses():
    dl = _dl()
    assert dl.TYPES['blur'] == BLUR and dl.BLUR_FIXED == BLUR_FIXED and dl.REFUSED_FAMILY == 6
    assert 9 not in dl.TYPES.values() and 11 not in dl.TYPES.values()
    assert dl.entry_params('blur', (2.0,)) == (13.0, 2.0) and dl.entry_params('blur', (0,)) == (0.0, 0.0)
    for code in (BLUR, BLUR_FIXED):
        geo = [(0, code, 37, 61, 3)] * 7
        par = [(0, 0.0), (4, 1.0), (33, 5.0), (3, 0.5), (31, 5.0), (-3, 1.0), (3.5, 1.0)]
        lay = dl.layout(geo, par)
        assert lay["status"].tolist() == [dl.REFUSED_SIZE, dl.REFUSED_OTHER, dl.REFUSED_OTHER, dl.OK, dl.OK,
                                          dl.REFUSED_OTHER, dl.REFUSED_OTHER]
        assert lay["out_off"].tolist()[:3] == [-1, -1, -1] and lay["out_hw"].tolist()[3] == [37, 61]
    # 9 and 11 stay "no type"
    lay = dl.layout([(0, 9, 8, 8, 3), (0, 11, 8, 8, 3)], [(3, 0.5)] * 2)
    assert lay["status"].tolist() == [dl.REFUSED_OTHER] * 2


def test_float_mode_refuses_what_another_family_serves_and_fixed_mode_takes_all():
    dl = _dl()
    assert [_ksize(r) // 2 for r in RADII] == [1, 3, 4, 6, 7, 9, 10, 12, 13, 15]         # the grid's ten radii
    entries = [(f, r) for f in range(len(SIZES)) for r in RADII]
    lay = _layout(entries)
    want = [expected_status(*SIZES[f], r) for f, r in entries]
    assert lay["status"].tolist() == want
    by_size = {hw: [lay["status"][j] for j, (f, _) in enumerate(entries) if SIZES[f] == hw] for hw in SIZES}
    assert by_size[(40, 352)] == [dl.REFUSED_FAMILY] * 10
    assert by_size[(40, 96)] == [dl.OK] * 3 + [dl.REFUSED_FAMILY] * 7           # R = 1, 3, 4 | 6 ...
    for hw in ((24, 96), (37, 61), (334, 500)):
        assert by_size[hw] == [dl.OK] * 10
    fixed = _layout(entries, BLUR_FIXED)
    assert not fixed["status"].any()
    _, rec, _ = dl.block_views(fixed["block"])
    assert set(rec["op"].tolist()) == {BLUR_FIXED}


def _mixed_entries():
    out = []
    for f in range(len(SIZES)):
        out += [(f, 'contrast', (0.5,)), (f, 'perspective_warp', ([1.0, 0, 0, 0, 1.0, 0, 0, 0],)), (f, 'scale', (1.1,))]
        out += [(f, r) for r in reversed(RADII)] + [(f, 2.0)]
    return out


@pytest.mark.parametrize("code", [BLUR, BLUR_FIXED])
def test_blur_units_come_last_sorted_in_bands_of_32_rows(code):
    dl = _dl()
    entries = _mixed_entries()
    lay = _layout(entries, code)
    hd, rec, units = dl.block_views(lay["block"])
    n_units, n_blur = int(hd["n_units"]), int(hd["n_blur"])
    assert 0 < n_blur < n_units and int(hd["n_plain"]) + int(hd["n_persp"]) < n_units - n_blur
    is_blur = np.isin(rec["op"][units["entry"]], (BLUR, BLUR_FIXED))
    assert not is_blur[:n_units - n_blur].any() and is_blur[n_units - n_blur:].all()
    tail = units[n_units - n_blur:]
    keys = [(int(rec["op"][e]), int(rec["ksx"][e])) for e in tail["entry"]]
    assert keys == sorted(keys) and len(set(keys)) == 10
    assert hd["lds_bytes"] <= dl.DRIVER_LIST_LDS_BYTES
    for j, ent in enumerate(entries):
        if len(ent) != 2:
            continue
        h, w = SIZES[ent[0]]
        mine = tail[tail["entry"] == j]
        if lay["status"][j]:
            assert len(mine) == 0 and lay["out_off"][j] == -1
            continue
        ks = _ksize(ent[1])
        assert rec[j]["op"] == code and rec[j]["ksx"] == rec[j]["ksy"] == ks and rec[j]["unit_rows"] == 32
        assert tuple(lay["out_hw"][j]) == (h, w) and lay["out_off"][j] % 48 == 0
        assert mine["y0"].tolist() == list(range(0, h, 32)) and mine["ny"].max() <= 32          # [0, h) exactly once
        assert (mine["y0"] + mine["ny"]).tolist() == mine["y0"].tolist()[1:] + [h]
        assert np.all(mine["lds_bytes"] == (32 + ks - 1) * 1024) and mine["lds_bytes"].max() <= 63488


def test_tables_are_shared_and_equal_the_dispatchers_taps():
    dl = _dl()
    entries = _mixed_entries()
    for code in (BLUR, BLUR_FIXED):
        lay = _layout(entries, code)
        _, rec, _ = dl.block_views(lay["block"])
        words = lay["block"].view(np.float32)
        tables = {}
        for j, ent in enumerate(entries):
            if len(ent) != 2 or lay["status"][j]:
                continue
            assert rec[j]["coeffs_x"] == rec[j]["coeffs_y"]
            tables.setdefault(ent[1], set()).add(int(rec[j]["coeffs_x"]))
        assert sorted(tables) == RADII
        assert all(len(v) == 1 for v in tables.values())      # equal (code, ksize, sigma): one table
        starts = sorted(next(iter(v)) for v in tables.values())
        assert len(set(starts)) == 10
        for radius, (at,) in ((r, tuple(v)) for r, v in tables.items()):
            ks = _ksize(radius)
            taps = words[at:at + ks]
            if code == BLUR:
                assert np.array_equal(taps, taps[::-1]) and abs(float(taps.astype(np.float64).sum()) - 1.0) < 1e-6
                assert np.allclose(taps, O.gaussian_kernel1d(ks, radius), rtol=2e-7, atol=0.0)
            else:
                assert np.array_equal(taps.astype(np.float64) * 256, O.gaussian_kernel_cv_fixed(ks, radius))
    # float and fixed entries of one (ksize, sigma) in one block have their own tables; sigma <= 0 takes the binomial table
    geo = [(3, BLUR, 37, 61, 3), (3, BLUR_FIXED, 37, 61, 3), (3, BLUR, 37, 61, 3), (3, BLUR_FIXED, 37, 61, 3)]
    lay = dl.layout(geo, [(5, 1.0), (5, 1.0), (5, 0.0), (5, -1.0)])
    _, rec, _ = dl.block_views(lay["block"])
    assert not lay["status"].any() and len(set(rec["coeffs_x"].tolist())) == 4
    words = lay["block"].view(np.float32)
    for j in (2, 3):
        assert words[rec[j]["coeffs_x"]:rec[j]["coeffs_x"] + 5].tolist() == [0.0625, 0.25, 0.375, 0.25, 0.0625]


def test_layouts_without_blur_are_unchanged():
    """No blur entry: n_blur (the former `reserved`) is 0, the units end with the resample section and the tables hold
    what the resample entries need, byte for byte where they were."""
    dl = _dl()
    others = [e for e in _mixed_entries() if len(e) == 3]
    lay = _layout(others)
    hd, rec, units = dl.block_views(lay["block"])
    assert hd["n_blur"] == 0 and dl._HEADER.itemsize == 48 and dl._HEADER.fields["n_blur"][1] == 44
    assert int(hd["n_units"]) == len(units) and rec["op"][units["entry"][-1]] == dl.TYPES['scale']
    # the same entries with blurs between them: the other sections' units and the resample tables do not move
    both = _layout(_mixed_entries())
    hd2, rec2, units2 = dl.block_views(both["block"])
    keep = [j for j, e in enumerate(_mixed_entries()) if len(e) == 3]
    n_other = int(hd2["n_units"]) - int(hd2["n_blur"])
    assert n_other == len(units) and (hd2["n_plain"], hd2["n_persp"], hd2["lds_bytes"]) == (hd["n_plain"], hd["n_persp"], hd["lds_bytes"])
    assert np.array_equal(np.asarray(keep)[units["entry"]], units2["entry"][:n_other])
    for name in ("y0", "ny", "lds_bytes"):
        assert np.array_equal(units[name], units2[name][:n_other])
    t1, t2 = int(hd["tables_off"]), int(hd2["tables_off"])
    used = max(int(r["coeffs_y"]) * 4 + int(r["win_h"]) * int(r["ksy"]) * 4 for r in rec if r["op"] == 0 and not r["status"]) - t1
    assert used > 0 and np.array_equal(lay["block"][t1:t1 + used], both["block"][t2:t2 + used])


def test_device_half_checks_the_blur_records_before_any_device_work():
    """imgxf_driver_list_u8 refuses a blur record that would let the kernel read taps outside the block, run with a
    radius it has no kernel for, or leave its entry — before it copies or launches anything (the pointers are never used)."""
    from imagetransformations_amd import _ffi
    dl = _dl()
    ents = [(3, 'contrast', (0.5,)), (3, 1.0), (4, 2.5), (3, 'scale', (1.1,)), (4, 0.5)]

    def run(change, code=BLUR):
        lay = _layout(ents, code)
        assert not lay["status"].any()
        hd, rec, units = dl.block_views(lay["block"])
        rec["src"], rec["src_stride"] = 4096, 1500
        change(hd, rec, units)
        return _ffi.lib.imgxf_driver_list_u8(lay["block"].ctypes.data, 4096, 4096, int(hd["out_bytes"]), None)

    def field(name, j, value):
        def change(hd, rec, units):
            rec[name][j] = value
        return change

    def header(name, value):
        def change(hd, rec, units):
            hd[name] = value
        return change

    def unit(name, k_from_end, value):
        def change(hd, rec, units):
            units[name][len(units) - 1 - k_from_end] = value
        return change

    def swap_runs(hd, rec, units):
        """The two neighbouring units at the first run boundary change places.  Each is moved whole, so it still is a
        valid band of its own entry, in the blur section, with its own LDS size: the run order alone is broken."""
        first = len(units) - int(hd["n_blur"])
        ks = rec["ksx"][units["entry"][first:]]
        b = first + int(np.flatnonzero(np.diff(ks))[0])
        assert ks[b - first] < ks[b - first + 1]
        units[[b, b + 1]] = units[[b + 1, b]]

    def into_the_resample_section(hd, rec, units):
        hd["n_blur"] = int(hd["n_blur"]) + 1
    bad = [_ffi.ERR_ARG, _ffi.ERR_SHAPE]
    for code in (BLUR, BLUR_FIXED):
        total_words = _layout(ents, code)["block"].nbytes // 4
        assert run(field("coeffs_x", 1, total_words - 3), code) in bad        # 7 taps, 3 words left
        assert run(field("coeffs_y", 2, total_words), code) in bad and run(field("coeffs_x", 4, 0), code) in bad
        assert run(field("coeffs_y", 1, -1), code) in bad
        assert run(field("ksx", 1, 8), code) in bad and run(field("ksx", 1, 33), code) in bad
        assert run(field("ksy", 2, 13), code) in bad and run(field("ksx", 4, 1), code) in bad
        assert run(field("unit_rows", 2, 16), code) in bad and run(field("oh", 2, 335), code) in bad
        assert run(header("n_blur", int(1e9)), code) in bad and run(header("n_blur", -1), code) in bad
        assert run(header("n_blur", 0), code) in bad and run(into_the_resample_section, code) in bad
        assert run(unit("y0", 0, 352), code) in bad and run(unit("ny", 0, 32), code) in bad
        assert run(unit("y0", 0, 8), code) in bad and run(unit("lds_bytes", 0, 1024), code) in bad
        assert run(unit("entry", 0, 0), code) in bad and run(swap_runs, code) in bad
