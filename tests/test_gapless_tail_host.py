"""fsgpu_gapless_item_records (host only, no GPU): the 16-byte device records the gapless scan makes of the planner's items.  The record carries, in
the top byte of its fourth word, the number of real columns of a stripe's last 16-column chunk (the trim), on the one item that ends with that
chunk; the other 24 + 32 bits are the stripe's offset in the scan layout, as before."""
import ctypes as C

import numpy as np
import pytest

from foldseek_amd import api


def _plan(chunks, ov, waves):
    L = api.lib()
    chunks = np.ascontiguousarray(chunks, np.uint32)
    n = L.fsgpu_gapless_plan_items(chunks.ctypes.data, len(chunks), ov, float(waves), None, 0, None)
    items = np.zeros(max(1, n), np.uint64)
    assert L.fsgpu_gapless_plan_items(chunks.ctypes.data, len(chunks), ov, float(waves), items.ctypes.data, n, None) == n
    return items[:n]


def _records(items, chunks, cols):
    L = api.lib()
    items = np.ascontiguousarray(items, np.uint64)
    chunks = np.ascontiguousarray(chunks, np.uint32)
    cols = np.ascontiguousarray(cols, np.uint32)
    rec = np.zeros((max(1, len(items)), 4), np.uint32)
    n = L.fsgpu_gapless_item_records(items.ctypes.data, len(items), chunks.ctypes.data, cols.ctypes.data, len(chunks), rec.ctypes.data)
    return n, rec[:len(items)]


def _fields(rec):
    trim = (rec[:, 3] >> np.uint32(24)).astype(np.int64)
    off = ((rec[:, 3] & np.uint32(0x00ffffff)).astype(np.uint64) << np.uint64(32)) | rec[:, 2].astype(np.uint64)
    return trim, off


def _offsets(chunks):
    """the stripe offsets of the scan layout (fsgpu_db_load): 8 uint4 per 16-column chunk, stripes back to back"""
    return np.concatenate(([0], np.cumsum(np.asarray(chunks, np.uint64) * np.uint64(8))[:-1])).astype(np.uint64)


@pytest.mark.parametrize("ov", [0, 1, 21, 56])
def test_trim_is_the_last_chunks_real_columns(ov):
    """stripes whose longest target ends 1, 4, 5, 15, 16 and 17 columns past a chunk boundary (17 = one column into the next chunk), at several
    stripe lengths, unsplit: every record carries longest target - 16 * (chunks - 1)"""
    cols = np.array([16 * base + past for base in (0, 1, 7, 30) for past in (1, 4, 5, 15, 16, 17)], np.uint32)
    chunks = (cols + 15) // 16
    items = _plan(chunks, ov, 1.0)                                                  # one wave: cutting a stripe only adds warm-up work
    assert len(items) == len(cols) and not ((items >> np.uint64(31)) & np.uint64(1)).any()
    n, rec = _records(items, chunks, cols)
    assert n == len(items)
    trim, off = _fields(rec)
    stripe = rec[:, 0].astype(np.int64)
    assert sorted(stripe.tolist()) == list(range(len(cols)))
    want = cols.astype(np.int64) - 16 * (chunks.astype(np.int64) - 1)
    assert (trim == want[stripe]).all() and set(trim.tolist()) == {1, 4, 5, 15, 16}
    assert (rec[:, 1] == (items & np.uint64(0xffffffff)).astype(np.uint32)).all()   # the range word is the planner's, untouched
    assert (rec[:, 0] == (items >> np.uint64(32)).astype(np.uint32)).all()
    assert (off == _offsets(chunks)[stripe]).all()


def test_only_the_last_segment_of_a_split_stripe_is_trimmed():
    """a 2000-column stripe among short ones, few waves: the planner cuts it into column segments; the segment that ends with the stripe's last
    chunk carries the trim, every other segment 0; all of them the stripe's own offset"""
    cols = np.array([40] * 50 + [2000] + [33] * 20 + [1999, 1985], np.uint32)
    chunks = (cols + 15) // 16
    for ov in (1, 8, 21):
        items = _plan(chunks, ov, 64.0)
        n, rec = _records(items, chunks, cols)
        assert n == len(items)
        trim, off = _fields(rec)
        stripe = rec[:, 0].astype(np.int64)
        split = (rec[:, 1] >> np.uint32(31)).astype(bool)
        end = (rec[:, 1] & np.uint32(0xffff)).astype(np.int64)
        assert (off == _offsets(chunks)[stripe]).all()
        for s in (50, 71, 72):                                                      # 2000 = 125 chunks of which the last is full, 1999, 1985 = one real column
            m = stripe == s
            assert m.sum() >= 2 and split[m].all(), (ov, s)
            last = m & (end == chunks[s])
            assert last.sum() == 1
            assert trim[last][0] == int(cols[s]) - 16 * (int(chunks[s]) - 1)
            assert (trim[m & ~last] == 0).all()
        whole = ~split
        assert (trim[whole] == (cols.astype(np.int64) - 16 * (chunks.astype(np.int64) - 1))[stripe[whole]]).all()
    assert {int(cols[s]) - 16 * (int(chunks[s]) - 1) for s in (50, 71, 72)} == {16, 15, 1}


def test_offsets_beyond_32_bits_and_refused_tables():
    """the offset keeps 56 bits: a table whose later stripes start beyond 2^32 uint4 comes back whole; tables that do not fit their items, or a
    chunk count that is not ceil(columns / 16), are refused"""
    chunks = np.full(70000, 0xffff, np.uint32)                                      # 70000 * 65535 * 8 uint4 > 2^35
    cols = chunks * np.uint32(16) - np.uint32(3)
    pick = np.array([0, 1, 8191, 8192, 8193, 69999], np.uint64)
    items = (pick << np.uint64(32)) | np.uint64(0xffff)
    n, rec = _records(items, chunks, cols)
    assert n == len(items)
    trim, off = _fields(rec)
    assert (trim == 13).all() and (off == _offsets(chunks)[pick.astype(np.int64)]).all() and int(off.max()) >> 32 > 0
    one = np.array([(0 << 32) | 3], np.uint64)
    assert _records(one, [3], [40])[0] == 1
    assert _records(one, [3], [49])[0] == -1                                        # 49 columns are 4 chunks
    assert _records(one, [2], [32])[0] == -1                                        # the item ends beyond its stripe
    assert _records(np.array([(5 << 32) | 3], np.uint64), [3], [40])[0] == -1      # no such stripe
    assert _records(np.zeros(0, np.uint64), [3], [40])[0] == 0
