"""Image-tile sharding restated in NumPy from the comments of include/mrirt.h (MrirtRenderExt::tileSize / tileRank / tileWorld /
tileSkew, mrirt_tiles_for_rank, mrirt_detile) and csrc/mrirt_device.h (map_pixel's three kinds).  TEST INFRASTRUCTURE ONLY; nothing
here is taken from mrirt/tiles.py, which tests/test_tiles_ref_host.py holds to this file.

The deal.  A W x H image is cut into tilesX x tilesY tiles of ts x ts pixels, tilesX = ceil(W / ts), tilesY = ceil(H / ts).  The
dealt tile t sits at row ty = t // tilesX, column tx = (t % tilesX + (skew % tilesX) * ty) % tilesX.  Rank r of `world` owns the
dealt tiles t = r, r + world, ... below tilesX * tilesY; its local tile lt is the dealt tile r + lt * world, i.e. lt = t // world.
A rank's compact buffer is [its tile count][ts][ts][4]; slots of an edge tile that lie outside the image hold the background with
alpha 1.  The gathered buffer is [world][max_local][ts][ts][4] with max_local = rank 0's count; the tiles a rank does not own (the
last one of the ranks that own one fewer, all of them for a rank beyond the tile count) are padding that never reaches the frame.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np


def tile_grid(w: int, h: int, ts: int) -> Tuple[int, int]:
    """(tilesX, tilesY)."""
    return -(-w // ts), -(-h // ts)


def tile_position(t: int, tiles_x: int, skew: int) -> Tuple[int, int]:
    """(tx, ty) of the dealt tile t."""
    ty = t // tiles_x
    tx = (t % tiles_x + (skew % tiles_x) * ty) % tiles_x
    return tx, ty


def tiles_of_rank(w: int, h: int, ts: int, rank: int, world: int) -> List[int]:
    """The dealt tiles a rank owns, in the order of its compact buffer."""
    tiles_x, tiles_y = tile_grid(w, h, ts)
    return list(range(rank, tiles_x * tiles_y, world))


def tiles_for_rank(w: int, h: int, ts: int, rank: int, world: int) -> int:
    return len(tiles_of_rank(w, h, ts, rank, world))


def max_local(w: int, h: int, ts: int, world: int) -> int:
    return tiles_for_rank(w, h, ts, 0, world)


def expected_compact(frame: np.ndarray, bg: Sequence[float], w: int, h: int, ts: int, rank: int, world: int, skew: int,
                     dtype=np.float32) -> np.ndarray:
    """The compact buffer rank `rank` must produce for the whole (h, w, 4) fp32 frame: in-image slots from the frame, off-image
    slots (bg, 1.0); for float16 the fp32 values rounded to nearest even, as the store's conversion does."""
    assert frame.shape == (h, w, 4) and frame.dtype == np.float32
    tiles_x, _ = tile_grid(w, h, ts)
    mine = tiles_of_rank(w, h, ts, rank, world)
    out = np.empty((len(mine), ts, ts, 4), np.float32)
    out[...] = np.array([bg[0], bg[1], bg[2], 1.0], np.float32)
    for lt, t in enumerate(mine):
        tx, ty = tile_position(t, tiles_x, skew)
        x0, y0 = tx * ts, ty * ts
        nx, ny = max(0, min(ts, w - x0)), max(0, min(ts, h - y0))
        out[lt, :ny, :nx] = frame[y0:y0 + ny, x0:x0 + nx]
    return out.astype(dtype)


def expected_frame(gathered: np.ndarray, w: int, h: int, ts: int, world: int, skew: int) -> np.ndarray:
    """The de-tiled (h, w, 4) frame of an arbitrary [world, max_local, ts, ts, 4] buffer: pixel by pixel, nothing but owned,
    in-image slots is read."""
    assert gathered.shape == (world, max_local(w, h, ts, world), ts, ts, 4), gathered.shape
    tiles_x, tiles_y = tile_grid(w, h, ts)
    out = np.empty((h, w, 4), gathered.dtype)
    for t in range(tiles_x * tiles_y):
        tx, ty = tile_position(t, tiles_x, skew)
        x0, y0 = tx * ts, ty * ts
        nx, ny = min(ts, w - x0), min(ts, h - y0)
        out[y0:y0 + ny, x0:x0 + nx] = gathered[t % world, t // world, :ny, :nx]
    return out


def synthetic_gathered(w: int, h: int, ts: int, world: int, dtype=np.float32) -> np.ndarray:
    """A gathered buffer that names its own slots: the four channels of owned slot (rank, lt, iy, ix) are
    (rank * max_local + lt, iy, ix, 7) — integers below 2048 at the sizes the tests use, exact in fp16 too — and every padded
    tile is NaN."""
    ml = max_local(w, h, ts, world)
    g = np.full((world, ml, ts, ts, 4), np.nan, np.float32)
    iy, ix = np.meshgrid(np.arange(ts, dtype=np.float32), np.arange(ts, dtype=np.float32), indexing="ij")
    for r in range(world):
        for lt in range(tiles_for_rank(w, h, ts, r, world)):
            g[r, lt, ..., 0] = r * ml + lt
            g[r, lt, ..., 1] = iy
            g[r, lt, ..., 2] = ix
            g[r, lt, ..., 3] = 7
    return g.astype(dtype)
