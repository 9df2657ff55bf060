"""Host half of `_list_block`, the code the list passes share: the slot and guard rule of an output allocation, the
predicate and the record address of a frame, and the entry validator of the resample passes — each against a plain
restatement written here.  No device."""
import numpy as np
import pytest
import torch

from imagetransformations_amd import _list_block as LB

SIZES = [1, 15, 16, 17, 48]


@pytest.mark.parametrize("guard", [0, 64])
def test_slots_are_16_byte_units_with_the_guard_around_each(guard):
    offs, total = LB.slots(SIZES, guard)
    pos, want = guard, []
    for nbytes in SIZES:                                      # the rule, restated: guard | slot | guard | slot ... | guard
        want.append(pos)
        pos += -(-nbytes // 16) * 16 + guard
    assert offs.tolist() == want and total == pos
    assert all(o % 16 == 0 for o in offs.tolist())
    ends = [o + -(-n // 16) * 16 for o, n in zip(offs.tolist(), SIZES)]
    assert offs[0] == guard and total - ends[-1] == guard
    assert [b - a for a, b in zip(ends, offs.tolist()[1:])] == [guard] * (len(SIZES) - 1)
    assert LB.slots([], guard)[1] == guard and LB.r16(17) == 32


def test_respace_moves_the_taken_entries_and_leaves_the_refused():
    taken = np.array([False, True, True, False, True, False])
    rec = np.zeros(6, np.dtype([("out_off", "<i8")]))
    hd = np.zeros(1, np.dtype([("out_bytes", "<u8")]))[0]
    rec["out_off"], hd["out_bytes"] = [-1, 0, 48, -1, 64, -1], 160         # as a layout gives them: slots of 48, 16, 96
    assert LB.respace(hd, rec, 64, taken) == 160 + 4 * 64 == int(hd["out_bytes"])
    assert rec["out_off"].tolist() == [-1, 64, 48 + 128, -1, 64 + 192, -1]
    assert LB.respace(hd, rec, 0, taken) == 416 and rec["out_off"][1] == 64
    rec["out_off"], hd["out_bytes"] = [0, 16, 32, 48, 64, 80], 96
    assert LB.respace(hd, rec, 16) == 96 + 7 * 16 and rec["out_off"].tolist() == [16, 48, 80, 112, 144, 176]


@pytest.mark.parametrize("guard", [-16, 8])
def test_guard_refusals(guard):
    with pytest.raises(ValueError, match="guard must be a non-negative multiple of 16"):
        LB.check_guard(guard)
    LB.check_guard(0), LB.check_guard(64)


def _dense(t, channels=3):
    return LB.rows_dense(t.shape, t.stride(), channels)


def test_rows_dense_and_addresses():
    flat = torch.arange(256, dtype=torch.uint8)
    one_row_0, one_row_7 = flat.as_strided((1, 5, 3), (0, 3, 1)), flat.as_strided((1, 5, 3), (7, 3, 1), 2)
    column = flat.as_strided((5, 1, 3), (3, 6, 1))                              # pixel stride 6: there is no second pixel
    cut = torch.zeros((4, 4, 4), dtype=torch.uint8)[:, :, :3]
    every_other = torch.zeros((4, 8, 3), dtype=torch.uint8)[:, ::2]
    gray = torch.zeros((3, 10), dtype=torch.uint8)
    assert _dense(one_row_0) and _dense(one_row_7) and _dense(column)
    assert not _dense(cut) and not _dense(every_other)
    small = torch.zeros((3, 5), dtype=torch.uint8)
    assert _dense(small, 1) and not _dense(small[:, ::2], 1)
    assert _dense(gray[:, :5], 1) and not _dense(gray[:, ::2], 1)
    ptr, stride = LB.addresses([one_row_0, one_row_7, column])
    assert ptr.dtype == np.uint64 and stride.dtype == np.int64
    assert ptr.tolist() == [flat.data_ptr(), flat.data_ptr() + 2, flat.data_ptr()] and stride.tolist() == [15, 15, 3]
    assert LB.address(one_row_7) == (flat.data_ptr() + 2, 15) and LB.address(column) == (flat.data_ptr(), 3)
    assert [a.tolist() for a in LB.addresses([gray[:, :5], gray[:1, :5]], 1)] == [[gray.data_ptr()] * 2, [10, 5]]
    for t in (one_row_0, column):                                              # read in place; a copy only where not dense
        assert LB.dense(t) is t
    copy = LB.dense(every_other)
    assert copy is not every_other and copy.is_contiguous() and torch.equal(copy, every_other)


# the texts the two callers hand the validator (resize_list.resize_list_block, tensor_maps.resized_crop_list)
FRAMES = [torch.zeros((6, 9, 3), dtype=torch.uint8), torch.zeros((4, 5, 3), dtype=torch.uint8)]
CALLERS = [("sizes has 3 rows for 2 frames (one per frame where no index is given)", ""),
           ("boxes has 3 rows for 2 entries (one per frame where no index is given)", " (torchvision pads there; not done here)")]


@pytest.mark.parametrize("rows,suffix", CALLERS)
def test_entries_validates_index_and_boxes_against_the_frames(rows, suffix):
    import re
    whole = np.array([[0, 0, 6, 9], [0, 0, 4, 5]], np.int64)
    index, hw, boxes = LB.entries(FRAMES, 2, None, None, rows, suffix)
    assert index.tolist() == [0, 1] and hw.tolist() == [[6, 9], [4, 5]] and np.array_equal(boxes, whole)
    index, hw, boxes = LB.entries(FRAMES, 3, np.array([1, 1, 0]), np.array([[3, 4, 1, 1], [0, 0, 4, 5], [5, 8, 1, 1]]), rows, suffix)
    assert hw.tolist() == [[4, 5], [4, 5], [6, 9]] and boxes[2].tolist() == [5, 8, 1, 1]
    with pytest.raises(ValueError, match=re.escape(rows)):                     # a wrong row count
        LB.entries(FRAMES, 3, None, None, rows, suffix)
    for bad in ([0, -1], [0, 2]):                                              # a negative index; one equal to len(frames)
        with pytest.raises(ValueError, match=re.escape("index values must lie in 0 .. 1")):
            LB.entries(FRAMES, 2, np.array(bad), None, rows, suffix)
    for box in ([1, 1, 0, 3], [-1, 0, 4, 5], [0, -1, 4, 5], [1, 0, 4, 5], [0, 1, 4, 5]):   # empty; one pixel out: top, left, bottom, right
        text = f"box {tuple(box)} (top, left, height, width) of entry 1 is empty or not inside its 4 x 5 frame{suffix}"
        with pytest.raises(ValueError, match=re.escape(text) + "$"):
            LB.entries(FRAMES, 2, None, np.array([[0, 0, 6, 9], box]), rows, suffix)
    assert LB.entries(FRAMES, 0, np.zeros(0, np.int64), np.zeros((0, 4), np.int64), rows, suffix)[1].shape == (0, 2)


# The Python halves restate the C records of include/imgxf.h as NumPy dtypes by hand: a block of two entries laid out by
# the library holds their sizes against the structs (the sections follow each other: header | records | units | tables)
def _two_entry_blocks():
    from imagetransformations_amd import background_list as BG, driver_list as DL, resize_list as RL, tensor_maps as TM
    frames = [(40, 52), (9, 130)]
    return {
        "driver_list": lambda: (DL.layout([[0, DL.TYPES['scale'], 40, 52, 3], [1, DL.TYPES['vert_flip'], 9, 130, 3]],
                                          [[1.25, 0.0], [0.0, 0.0]])["block"], DL._HEADER, DL._ENTRY, DL._UNIT, "entries"),
        "resize_list": lambda: (RL.layout([[40, 52, 0, 0, 40, 52, 20, 31], [9, 130, 1, 2, 7, 100, 12, 64]]),
                                RL._HEADER, RL._ENTRY, RL._UNIT, "entries"),
        "background_list": lambda: (BG.layout([[40, 52, 1, 2, 3], [9, 130, 4, 5, 6]]), BG._HEADER, BG._ENTRY, BG._UNIT, "entries"),
        "preprocess_list": lambda: (TM.preprocess_layout(TM.preprocess_geometry(frames, 32, 24), 24),
                                    TM._PL_HEADER, TM._PL_FRAME, TM._PL_UNIT, "frames"),
        "resized_crop_list": lambda: (TM.resized_crop_layout(np.array([[40, 52, 3, 4, 30, 40, 0], [9, 130, 0, 0, 9, 130, 1]], np.int32),
                                                             (24, 20)), TM._RCL_HEADER, TM._RCL_ENTRY, TM._RCL_UNIT, "entries"),
    }


@pytest.mark.parametrize("name", ["driver_list", "resize_list", "background_list", "preprocess_list", "resized_crop_list"])
def test_python_record_dtypes_have_the_sizes_of_the_c_structs(name):
    block, header, record, unit, records = _two_entry_blocks()[name]()
    hd = block[:header.itemsize].view(header)[0]
    n_units, records_off, units_off = int(hd["n_units"]), int(hd[records + "_off"]), int(hd["units_off"])
    assert int(hd["n_" + records]) == 2 and n_units >= 2
    assert records_off == header.itemsize
    assert units_off - records_off == 2 * record.itemsize
    units_end = units_off + n_units * unit.itemsize
    if "tables_off" in header.names:
        assert int(hd["tables_off"]) == units_end
    assert int(hd["total_bytes"]) == block.nbytes >= units_end and block.nbytes % 16 == 0
    if "tables_off" not in header.names:
        assert block.nbytes - units_end < 16                                   # no tables: the units end the block
    rec, units = LB.views(block, header, record, unit, records)[1:]
    first = "frame" if records == "frames" else "entry"
    assert len(units) == n_units and sorted(set(units[first].tolist())) == [0, 1]
    assert rec["h"].tolist() == [40, 9] and rec["w"].tolist() == [52, 130]
