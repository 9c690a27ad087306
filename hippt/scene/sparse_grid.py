"""Sparse bricked density/temperature grids.

A `SparseGrid` stores a (nz, ny, nx) float32 volume as the list of its
non-empty 8^3 bricks: `coords` names the resident bricks, `values` holds
their voxels, everything else is background 0.  The brick edge matches the
NanoVDB leaf size, so .nvdb leaves map onto bricks without resampling and
the device lookup (csrc/core/medium.h) is shifts and masks:

    b = table[((iz>>3)*bny + (iy>>3))*bnx + (ix>>3)]        # -1 = empty
    v = b < 0 ? 0 : pool[b*512 + ((iz&7)<<6 | (iy&7)<<3 | (ix&7))]

The brick table is dense over ceil(n/8) cells per axis (1/128 of the dense
grid's bytes), so memory is table + supergrid + resident bricks: bounded far
below the dense grid, but not strictly proportional to occupancy.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

BRICK = 8


def brick_dims(shape) -> Tuple[int, int, int]:
    """Brick-table extent (bnz, bny, bnx) of a (nz, ny, nx) grid."""
    return tuple((int(n) + BRICK - 1) // BRICK for n in shape)


class SparseGrid:
    """Plain container: `shape` (nz, ny, nx); `coords` (n, 3) int32 brick
    coordinates (bz, by, bx), unique and lexicographically sorted; `values`
    (n, 8, 8, 8) float32 in (z, y, x) order.  Edge bricks of grids whose dims
    are not multiples of 8 are zero-padded; background is always 0."""

    BRICK = BRICK

    def __init__(self, shape, coords, values):
        shape = tuple(int(n) for n in shape)
        if len(shape) != 3 or min(shape) <= 0:
            raise ValueError(f"shape must be three positive dims (nz, ny, nx), got {shape}")
        coords = np.ascontiguousarray(np.asarray(coords, np.int32).reshape(-1, 3))
        values = np.ascontiguousarray(
            np.asarray(values, np.float32).reshape(-1, BRICK, BRICK, BRICK))
        if len(coords) != len(values):
            raise ValueError(f"{len(coords)} brick coords but {len(values)} bricks")
        bd = brick_dims(shape)
        if len(coords):
            if coords.min() < 0 or (coords >= np.asarray(bd, np.int32)).any():
                raise ValueError(f"brick coords outside the {bd} brick table")
            keys = _keys(coords, bd)
            if (np.diff(keys) <= 0).any():
                order = np.argsort(keys, kind="stable")
                keys = keys[order]
                if (np.diff(keys) == 0).any():
                    raise ValueError("duplicate brick coords")
                coords = np.ascontiguousarray(coords[order])
                values = np.ascontiguousarray(values[order])
        self.shape = shape
        self.coords = coords
        self.values = values

    # ------------------------------------------------------------ builders
    @classmethod
    def from_dense(cls, arr) -> "SparseGrid":
        """Keep a brick iff any voxel in it is nonzero."""
        a = np.ascontiguousarray(np.asarray(arr, np.float32))
        if a.ndim != 3:
            raise ValueError("density must be (nz, ny, nx)")
        nz, ny, nx = a.shape
        bz, by, bx = brick_dims(a.shape)
        ap = np.pad(a, ((0, bz * BRICK - nz), (0, by * BRICK - ny), (0, bx * BRICK - nx)))
        blocks = ap.reshape(bz, BRICK, by, BRICK, bx, BRICK).transpose(0, 2, 4, 1, 3, 5)
        keep = (blocks != 0).any(axis=(3, 4, 5))
        coords = np.argwhere(keep).astype(np.int32)          # sorted (bz, by, bx)
        return cls(a.shape, coords, blocks[keep])

    @classmethod
    def from_bricks(cls, shape, bricks: Dict[Tuple[int, int, int], np.ndarray]) -> "SparseGrid":
        """Build from a {(bz, by, bx): (8, 8, 8) array} dict; all-zero bricks
        are dropped."""
        items = [(k, v) for k, v in bricks.items() if np.any(v)]
        if not items:
            return cls(shape, np.zeros((0, 3), np.int32),
                       np.zeros((0, BRICK, BRICK, BRICK), np.float32))
        coords = np.asarray([k for k, _ in items], np.int32)
        values = np.stack([np.asarray(v, np.float32) for _, v in items])
        return cls(shape, coords, values)

    # ------------------------------------------------------------- queries
    @property
    def n_bricks(self) -> int:
        return int(len(self.coords))

    @property
    def brick_dims(self) -> Tuple[int, int, int]:
        return brick_dims(self.shape)

    @property
    def occupancy(self) -> float:
        """Fraction of the brick table's cells that are resident."""
        bd = self.brick_dims
        return self.n_bricks / float(bd[0] * bd[1] * bd[2])

    @property
    def nbytes(self) -> int:
        return int(self.coords.nbytes + self.values.nbytes)

    @property
    def dense_nbytes(self) -> int:
        return 4 * self.shape[0] * self.shape[1] * self.shape[2]

    def to_dense(self) -> np.ndarray:
        nz, ny, nx = self.shape
        bz, by, bx = self.brick_dims
        blocks = np.zeros((bz, by, bx, BRICK, BRICK, BRICK), np.float32)
        c = self.coords
        blocks[c[:, 0], c[:, 1], c[:, 2]] = self.values
        full = blocks.transpose(0, 3, 1, 4, 2, 5).reshape(bz * BRICK, by * BRICK, bx * BRICK)
        return np.ascontiguousarray(full[:nz, :ny, :nx])

    def reindexed(self, coords) -> np.ndarray:
        """This grid's bricks laid out over `coords` (a sorted superset of
        self.coords): (len(coords), 8, 8, 8), zeros where this grid has no
        brick.  Lets two grids share one brick table."""
        coords = np.asarray(coords, np.int32).reshape(-1, 3)
        out = np.zeros((len(coords), BRICK, BRICK, BRICK), np.float32)
        if self.n_bricks:
            bd = self.brick_dims
            pos = np.searchsorted(_keys(coords, bd), _keys(self.coords, bd))
            out[pos] = self.values
        return out

    def __repr__(self):
        return (f"SparseGrid(shape={self.shape}, n_bricks={self.n_bricks}, "
                f"occupancy={self.occupancy:.4f})")


def _keys(coords, bd) -> np.ndarray:
    c = coords.astype(np.int64)
    return (c[:, 0] * bd[1] + c[:, 1]) * bd[2] + c[:, 2]


def union_coords(a: SparseGrid, b: SparseGrid) -> np.ndarray:
    """Sorted union of two grids' brick coordinates (same shape required)."""
    if a.shape != b.shape:
        raise ValueError(f"grid shapes differ: {a.shape} vs {b.shape}")
    bd = a.brick_dims
    keys = np.union1d(_keys(a.coords, bd), _keys(b.coords, bd))
    out = np.empty((len(keys), 3), np.int32)
    out[:, 2] = keys % bd[2]
    out[:, 1] = (keys // bd[2]) % bd[1]
    out[:, 0] = keys // (bd[2] * bd[1])
    return out
