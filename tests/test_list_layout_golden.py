"""The host blocks of the five record-driven list passes, byte for byte: every layout of the seeded corpus of
tests/golden/make_list_layout_golden.py against the digests that file wrote once (tests/golden/list_layout_digests.json).
The host halves are pure functions of their inputs, so any differing byte is a defect.  The corpus is held to what makes
it worth hashing — small frames, one-pixel and tall boxes, shared geometries, every driver type accepted, every refusal
status drawn — so that it cannot degenerate unnoticed.  No device."""
import importlib.util
import json
import os

import numpy as np
import pytest

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_list_layout_golden.py")
_spec = importlib.util.spec_from_file_location("make_list_layout_golden", _PATH)
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def corpus():
    return G.corpus()


@pytest.fixture(scope="module")
def golden():
    with open(G.PATH) as f:
        return json.load(f)


def test_every_block_equals_its_digest(corpus, golden):
    got = G.digests(corpus)
    assert sorted(got) == sorted(golden)
    differing = {k: (got[k], golden[k]) for k in golden if got[k] != golden[k]}
    assert not differing


def test_parameter_sets(golden):
    want = [f"driver_list/{b}" for b in (65536, 20000, 3000)]
    want += [f"{p}/{f}" for p in ("resize_list", "preprocess_list") for f in ("BILINEAR", "BICUBIC", "LANCZOS")]
    want += [f"resized_crop_list/{f}/{s}" for f in ("BILINEAR", "BICUBIC", "BOX") for s in ("224x224", "7x5")]
    want += ["background_list"]
    assert all(k in golden for k in want)
    for p in ("driver_list", "resize_list", "preprocess_list", "resized_crop_list", "background_list"):
        assert any(k.startswith(p) and k.endswith("/n0") for k in golden)
    assert golden["background_list/n0"]["bytes"] == 48         # the header alone, rounded to 16


def test_corpus_geometry(corpus):
    g = corpus["resize_list"]
    h, w, bh, bw, oh, ow = g[:, 0], g[:, 1], g[:, 4], g[:, 5], g[:, 6], g[:, 7]
    assert len(g) == G.N >= 1000
    assert h.min() == 1 and w.min() == 1 and 500 <= h.max() <= G.SIDE and 500 <= w.max() <= G.SIDE
    assert 0.15 * G.N <= (h < 9).sum() <= 0.3 * G.N                            # a fifth of the frames
    assert ((bh == 1) & (bw == 1)).sum() >= 16
    tall = (bh.astype(np.int64) > bw.astype(np.int64) * 100)
    assert (tall & (oh < bh)).sum() >= 16                                      # resize_list refuses these: rows first
    assert (tall & (bh > 224)).sum() >= 16 and (tall & (bh > 7)).sum() >= 16   # resized_crop_list's `tall` entries
    for a in (w, bw, ow):
        assert (a % 4 == 0).sum() >= 64 and (a % 4 != 0).sum() >= 64
    for name in ("resize_list", "resized_crop_list", "preprocess_list", "background_list"):
        rows = corpus[name]
        assert len(rows) == G.N and len(np.unique(rows, axis=0)) <= G.N - 64   # repeated geometries: tables are shared
    # axes in common between entries of different geometry, too (resize_list and driver_list key tables per axis)
    assert len({(a, b) for a, b in zip(bw.tolist(), ow.tolist())}) < len(np.unique(g[:, 4:], axis=0))


def test_driver_corpus_draws_every_type_and_every_refusal(corpus):
    from imagetransformations_amd import driver_list as DL
    geo, p = corpus["driver_list"]
    status = {b: DL.layout(geo, p, b)["status"] for b in G.BUDGETS}
    ok = status[65536] == DL.OK
    codes = sorted(set(DL.TYPES.values()) | {DL.BLUR_FIXED})
    assert codes == list(G.DRIVER_TYPES)
    for code in codes:
        assert (ok & (geo[:, 1] == code)).sum() >= 8, code
    seen = np.concatenate(list(status.values()))
    for st in (DL.OK, DL.REFUSED_LDS, DL.REFUSED_SIZE, DL.REFUSED_TURN, DL.REFUSED_FORMAT, DL.REFUSED_OTHER, DL.REFUSED_FAMILY):
        assert (seen == st).sum() >= 1, st
    assert (status[3000] == DL.REFUSED_LDS).sum() > (status[20000] == DL.REFUSED_LDS).sum() >= (status[65536] == DL.REFUSED_LDS).sum()
    for code in (DL.TYPES['blur'], DL.BLUR_FIXED):
        assert len(set(p[ok & (geo[:, 1] == code), 0].tolist())) >= 3, code    # radii, as kernel sizes
    assert ok.sum() >= 0.6 * G.N
