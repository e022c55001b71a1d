"""tests/tiles_ref.py (the tile deal restated from include/mrirt.h) against the library's host side: mrirt_tiles_for_rank,
tiles.local_tile_count, tiles.tile_origin and the host branch of tiles.assemble_frame — and against itself: every rank's tiles
partition the tile grid, and what expected_compact deals out expected_frame puts back.  No GPU."""
import itertools

import numpy as np
import pytest

import tiles_ref as R

# (w, h, ts): ragged in both directions, narrower than one tile, one pixel, exact multiples, a wide grid
SIZES = [(40, 28, 16), (40, 28, 32), (40, 28, 48), (10, 40, 16), (1, 1, 16), (64, 32, 16), (128, 48, 16), (130, 70, 32), (49, 33, 16)]
WORLDS = [1, 2, 3, 4, 5, 8, 13, 32]
BG = (0.125, 0.5, 0.75)


def _skews(tiles_x):
    return sorted({0, 1, 2, 5, max(tiles_x - 1, 0), tiles_x, tiles_x + 1, 3 * tiles_x + 2})


def test_the_grid_spans_what_it_claims():
    seen = set()
    for (w, h, ts), world in itertools.product(SIZES, WORLDS):
        tx, ty = R.tile_grid(w, h, ts)
        seen |= {"narrow" if w < ts else "", "empty ranks" if world > tx * ty else "",
                 "columns" if world > 1 and tx > 1 and tx % world == 0 else "", "no columns" if world > 1 and tx % world != 0 else ""}
        assert any(s >= tx for s in _skews(tx))
    assert {"narrow", "empty ranks", "columns", "no columns"} <= seen


def test_a_deal_worked_by_hand():
    """40 x 28 at tile 16: a 3 x 2 grid; skew 2 rotates row 1 by two columns; rank 0 of 3 owns dealt tiles 0 and 3."""
    assert R.tile_grid(40, 28, 16) == (3, 2)
    assert [R.tile_position(t, 3, 2) for t in range(6)] == [(0, 0), (1, 0), (2, 0), (2, 1), (0, 1), (1, 1)]
    assert [R.tile_position(t, 3, 5) for t in range(6)] == [R.tile_position(t, 3, 2) for t in range(6)]
    assert R.tiles_of_rank(40, 28, 16, 0, 3) == [0, 3] and R.tiles_of_rank(40, 28, 16, 6, 7) == []
    frame = np.arange(28 * 40 * 4, dtype=np.float32).reshape(28, 40, 4)
    c = R.expected_compact(frame, BG, 40, 28, 16, 0, 3, 2)
    assert c.shape == (2, 16, 16, 4)
    assert np.array_equal(c[0], frame[0:16, 0:16])
    assert np.array_equal(c[1, :12, :8], frame[16:28, 32:40])                    # the corner tile: 8 columns and 12 rows in the image
    off = np.ones((16, 16), bool)
    off[:12, :8] = False
    assert np.array_equal(c[1][off], np.tile(np.array(BG + (1.0,), np.float32), (off.sum(), 1)))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-t%d" % s)
def test_counts_origins_and_partition(size):
    from mrirt import render, tiles
    w, h, ts = size
    tiles_x, tiles_y = R.tile_grid(w, h, ts)
    assert tiles.num_tiles(w, h, ts) == tiles_x * tiles_y
    for world in WORLDS:
        counts = [R.tiles_for_rank(w, h, ts, r, world) for r in range(world)]
        assert sum(counts) == tiles_x * tiles_y and max(counts) == counts[0] == R.max_local(w, h, ts, world)
        assert max(counts) - min(counts) <= 1
        for r in range(world):
            assert render.tiles_for_rank(w, h, ts, r, world) == counts[r], (world, r)          # lib.mrirt_tiles_for_rank
            assert tiles.local_tile_count(w, h, ts, r, world) == counts[r], (world, r)
        for skew in _skews(tiles_x):
            where = {}
            for r in range(world):
                for lt, t in enumerate(R.tiles_of_rank(w, h, ts, r, world)):
                    assert t // world == lt and t % world == r
                    tx, ty = R.tile_position(t, tiles_x, skew)
                    assert tiles.tile_origin(t, w, ts, skew) == (tx * ts, ty * ts), (world, skew, t)
                    assert (tx, ty) not in where, f"tile {(tx, ty)} dealt twice: {where[(tx, ty)]} and {(r, lt)}"
                    where[(tx, ty)] = (r, lt)
            assert set(where) == set(itertools.product(range(tiles_x), range(tiles_y))), (world, skew)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-t%d" % s)
def test_frames_round_trip_and_the_host_branch_agrees(size):
    import torch
    from mrirt import tiles
    w, h, ts = size
    tiles_x, _ = R.tile_grid(w, h, ts)
    rng = np.random.default_rng(w * 1000 + h * 10 + ts)
    frame = rng.random((h, w, 4), dtype=np.float32)
    for world in WORLDS:
        ml = R.max_local(w, h, ts, world)
        synth = R.synthetic_gathered(w, h, ts, world)
        for skew in _skews(tiles_x):
            # what the ranks must render, padded with NaN, comes back as the frame
            g = np.full((world, ml, ts, ts, 4), np.nan, np.float32)
            inside = 0
            for r in range(world):
                c = R.expected_compact(frame, BG, w, h, ts, r, world, skew)
                assert c.shape == (R.tiles_for_rank(w, h, ts, r, world), ts, ts, 4) and np.all(c[..., 3][c[..., 0] == BG[0]] == 1.0)
                inside += int((c[..., :3] != np.array(BG, np.float32)).any(axis=-1).sum())
                g[r, :c.shape[0]] = c
                h16 = R.expected_compact(frame, BG, w, h, ts, r, world, skew, dtype=np.float16)
                assert h16.dtype == np.float16 and np.array_equal(h16, c.astype(np.float16))
            assert inside == w * h                       # (random colours in (0, 1): none equals the background)
            assert np.array_equal(R.expected_frame(g, w, h, ts, world, skew), frame), (world, skew)
            # the host branch of assemble_frame, on the random frame's tiles and on the buffer that names its slots
            for buf in (g, synth):
                want = R.expected_frame(buf, w, h, ts, world, skew)
                assert not np.isnan(want).any()
                got = tiles.assemble_frame(torch.from_numpy(buf), w, h, ts, world, skew).numpy()
                assert got.shape == (h, w, 4) and np.array_equal(got, want), (world, skew)
        # the synthetic buffer: every pixel names the slot the deal gives it
        want = R.expected_frame(synth, w, h, ts, world, 1)
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        assert np.array_equal(want[..., 1], ys % ts) and np.array_equal(want[..., 2], xs % ts) and np.all(want[..., 3] == 7)
