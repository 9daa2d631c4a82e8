"""CPU checks of what lies between the trace walk and the caller's transcript arena in the device half of the extension stage
(diamond_amd/csrc/transcript_core.h, extend_core.h tr_layout; via tests/emu/libswipe_emu.so, tests/emu/transcript_emu.cpp):
 * the layout of the transcript arrays over the shape grid of tests/test_extend_layout.py: every region inside the buffer;
 * the arithmetic the ext_tr_* kernels use, lane by lane: raw slots never overlap and never leave their piece, a piece holds as many
   consecutive entries as fit the limit and at least one, keep followed by gather reproduces every record's transcript with its
   terminator at a dense offset in record order under a random record -> slot map, and the gathered size is the sum of len + 1."""
import ctypes

import numpy as np
import pytest

import emu_py as emu
from test_extend_layout import SHAPES

MAX_REGIONS = 16
u64, i64, u32, i32 = ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int32
vp = ctypes.c_void_p


def tr_layout(n_groups, walk_cap, record_cap):
    lib = emu.lib()
    names = (ctypes.c_char_p * MAX_REGIONS)()
    off, used = np.zeros(MAX_REGIONS, np.uint64), np.zeros(MAX_REGIONS, np.uint64)
    total = u64(0)
    lib.emu_tr_layout.argtypes = [u64, u64, u64, ctypes.c_int, vp, vp, vp, ctypes.POINTER(u64)]
    n = lib.emu_tr_layout(n_groups, walk_cap, record_cap, MAX_REGIONS, ctypes.cast(names, vp), off.ctypes.data, used.ctypes.data, ctypes.byref(total))
    assert 0 < n <= MAX_REGIONS
    return [(names[i].decode(), int(off[i]), int(used[i])) for i in range(n)], total.value


@pytest.mark.parametrize("mode", ["k", "filters", "top"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_every_transcript_array_lies_inside_its_region(shape, mode):
    """The capacities are those of ext_layout for the same call: records min(groups, queries x k), or the groups under --top; the
    walked list the records', or the groups with HSP filters or --top."""
    n_groups, n_queries, _, k = SHAPES[shape]
    n_rec = n_groups if mode == "top" else min(n_groups, n_queries * k)
    n_walk = n_rec if mode == "k" else n_groups
    regions, total = tr_layout(n_groups, n_walk, n_rec)
    names = [r[0] for r in regions]
    assert len(set(names)) == len(names)
    for i, (name, off, used) in enumerate(regions):
        end = regions[i + 1][1] if i + 1 < len(regions) else total
        assert off % 64 == 0, name
        assert off + used <= end, f"{name}: {off + used - end} bytes past its region"
    got = dict((r[0], r[2]) for r in regions)
    assert got["g_store"] >= n_groups * 8
    assert got["k_len"] >= (n_walk + 1) * 8 and got["k_off"] >= (n_walk + 1) * 8      # (the scans write entries + 1)
    assert got["r_len"] >= (n_rec + 1) * 8 and got["r_off"] >= (n_rec + 1) * 8
    assert got["pieces"] >= (n_walk + 1) * 4                                             # (one piece per entry at the most)
    assert got["tr_ctr"] > 0


def test_slot_bound_and_kept_bytes():
    lib = emu.lib()
    lib.emu_tr_slot_bytes.restype = i64
    lib.emu_tr_kept_bytes.restype = i64
    assert lib.emu_tr_slot_bytes(i32(300), i32(250)) == 552
    assert lib.emu_tr_slot_bytes(i32(2**31 - 1), i32(2**31 - 1)) == 2**32                # (64-bit: no wrap)
    assert [lib.emu_tr_kept_bytes(i32(x)) for x in (-1, 0, 1, 551)] == [1, 1, 2, 552]


def _pieces(widths, limit):
    lib = emu.lib()
    w = np.ascontiguousarray(widths, np.int64)
    bounds, scan = np.zeros(len(w) + 1, np.uint32), np.zeros(len(w) + 1, np.int64)
    lib.emu_tr_pieces.argtypes = [vp, u32, i64, vp, vp]
    lib.emu_tr_pieces.restype = u32
    n = lib.emu_tr_pieces(w.ctypes.data, len(w), limit, bounds.ctypes.data, scan.ctypes.data)
    return bounds[:n + 1].tolist(), scan


@pytest.mark.parametrize("limit", [1, 99, 100, 101, 250, 1000, 10**9])
def test_pieces_are_maximal_runs_that_fit_the_limit_with_one_entry_at_least(limit):
    rng = np.random.default_rng(limit)
    widths = rng.integers(2, 200, 500)
    widths[::50] = 100
    bounds, scan = _pieces(widths, limit)
    assert bounds[0] == 0 and bounds[-1] == len(widths)
    for b, e in zip(bounds, bounds[1:]):
        assert e > b
        size = int(scan[e] - scan[b])
        assert size <= limit or e == b + 1                    # fits, or is one entry wider than the limit on its own
        if e < len(widths):
            assert size + int(widths[e]) > limit              # ... and the next entry would not have fitted
    assert _pieces([7], 1)[0] == [0, 1]
    assert _pieces([], 100)[0] == [0]


def _keep_gather(qlen, tlen, lens, limit, slot_of, rng, store_cap=None, out_cap=None):
    lib = emu.lib()
    n = len(lens)
    tr_at = np.zeros(n, np.int64)
    tr_at[1:] = np.cumsum(lens[:-1])
    tr = rng.integers(1, 256, int(lens.sum()) + 1).astype(np.uint8)            # (no 0 byte inside a transcript)
    total_kept = int(lens.sum()) + n
    total_out = int(lens[slot_of].sum()) + len(slot_of)
    store_cap = total_kept if store_cap is None else store_cap
    out_cap = total_out if out_cap is None else out_cap
    store, out = np.full(store_cap + 64, 0xA5, np.uint8), np.full(out_cap + 64, 0xA5, np.uint8)
    store_off, rec_off, sizes = np.zeros(n, np.int64), np.zeros(len(slot_of), np.int64), np.zeros(5, np.int64)
    q, t, l = (np.ascontiguousarray(x, np.int32) for x in (qlen, tlen, lens))
    s = np.ascontiguousarray(slot_of, np.uint32)
    lib.emu_tr_keep_gather.argtypes = [u32, vp, vp, vp, vp, vp, i64, u32, vp, vp, i64, vp, vp, i64, vp, vp]
    rc = lib.emu_tr_keep_gather(n, q.ctypes.data, t.ctypes.data, l.ctypes.data, tr.ctypes.data, tr_at.ctypes.data, limit, len(s), s.ctypes.data,
                                store.ctypes.data, store_cap, store_off.ctypes.data, out.ctypes.data, out_cap, rec_off.ctypes.data, sizes.ctypes.data)
    return rc, tr, tr_at, store, store_off, out, rec_off, sizes, total_kept, total_out


@pytest.mark.parametrize("limit", [1, 700, 5000, 10**9], ids=["one_entry_per_piece", "few_entries_per_piece", "several_pieces", "one_piece"])
def test_keep_then_gather_reproduces_every_transcript_in_record_order(limit):
    rng = np.random.default_rng(5)
    n = 400
    qlen, tlen = rng.integers(1, 400, n), rng.integers(1, 400, n)
    lens = rng.integers(0, 300, n)
    lens = np.minimum(lens, qlen + tlen)
    lens[:8] = 0                                              # empty transcripts: the terminator alone
    lens[8:16] = (qlen + tlen)[8:16]                          # ... and transcripts at the slot bound (+ terminator = the slot less one byte)
    perm = rng.permutation(n)
    qlen, tlen, lens = qlen[perm], tlen[perm], lens[perm]
    slot_of = rng.permutation(n)[:300]                        # a random record -> slot map; 100 walked entries are no record
    rc, tr, tr_at, store, store_off, out, rec_off, sizes, total_kept, total_out = _keep_gather(qlen, tlen, lens, limit, slot_of, rng)
    assert rc == 0
    pieces, raw_max, kept, gathered, bad = sizes.tolist()
    assert bad == 0, "raw slots overlap or leave their piece"
    widths = qlen + tlen + 2
    assert raw_max <= max(limit, int(widths.max()))
    assert pieces == len(_pieces(widths, limit)[0]) - 1
    if limit == 1:
        assert pieces == n
    if limit == 10**9:
        assert pieces == 1
    # the store: dense, in the order of the walked list, whatever the pieces
    assert kept == total_kept
    assert store_off.tolist() == (np.concatenate([[0], np.cumsum(lens + 1)[:-1]])).tolist()
    # the output: dense, in record order, each transcript with its terminator; nothing behind it touched
    assert gathered == total_out == int(lens[slot_of].sum()) + len(slot_of)
    assert rec_off.tolist() == (np.concatenate([[0], np.cumsum(lens[slot_of] + 1)[:-1]])).tolist()
    for r, s in enumerate(slot_of):
        want = np.concatenate([tr[tr_at[s]: tr_at[s] + lens[s]], np.zeros(1, np.uint8)])
        assert np.array_equal(out[rec_off[r]: rec_off[r] + lens[s] + 1], want), (r, s)
    assert (store[kept:] == 0xA5).all() and (out[gathered:] == 0xA5).all()


def test_an_output_or_a_store_one_byte_short_is_refused_and_left_alone():
    rng = np.random.default_rng(9)
    n = 50
    qlen, tlen = rng.integers(10, 100, n), rng.integers(10, 100, n)
    lens = rng.integers(0, 20, n)
    slot_of = np.arange(n)[::-1].copy()
    total_out = int(lens.sum()) + n
    rc, *_, out, _, sizes, _, _ = _keep_gather(qlen, tlen, lens, 10**9, slot_of, np.random.default_rng(1), out_cap=total_out - 1)
    assert rc == -1 and (out == 0xA5).all()
    rc = _keep_gather(qlen, tlen, lens, 10**9, slot_of, np.random.default_rng(1), store_cap=total_out - 1)[0]
    assert rc == -1
