"""Analytic exchange oracles shared by the tests and the GPU validation scripts.

Same idea as the reference's tests (test/test_exchange.cu:12-38 "ripple", test_cuda_mpi_distributed_domain.cu:10-22
coordinate packing): every interior cell holds a function of its global coordinate; after exchange() every halo
cell in direction d must hold the value at its periodic image iff radius(d) != 0, and keep its poison otherwise.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _C

POISON = -1
POISON_BYTE = 0xFF


def encode(gz, gy, gx):
    return gx + 1000 * gy + 1000000 * gz


def fill_coords(dd, q: int, poison: int = POISON, offset: int = 0):
    """Poison whole allocations (curr and next), then write encode(global coord) + offset into every interior cell."""
    for di in range(dd.num_domains()):
        for curr in (True, False):
            t = dd.curr(di, q) if curr else dd.next(di, q)
            t.fill_(poison)
    dd.fill_from_global(q, lambda z, y, x: encode(z, y, x) + offset)


def expected_full(dd, di: int, radius, poison: int = POISON, boundary=None, offset: int = 0) -> torch.Tensor:
    d = dd.domain(di)
    org, raw, sz = d.accessor_origin(), d.raw_size(), d.size()
    cr = d.get_compute_region()
    Z, Y, X = dd.size().z, dd.size().y, dd.size().x
    gz = torch.arange(raw.z).view(-1, 1, 1) + org.z
    gy = torch.arange(raw.y).view(1, -1, 1) + org.y
    gx = torch.arange(raw.x).view(1, 1, -1) + org.x
    dz = (gz >= cr.hi.z).long() - (gz < cr.lo.z).long()
    dy = (gy >= cr.hi.y).long() - (gy < cr.lo.y).long()
    dx = (gx >= cr.hi.x).long() - (gx < cr.lo.x).long()
    dz, dy, dx = torch.broadcast_tensors(dz, dy, dx)
    want = (encode(gz % Z, gy % Y, gx % X) + offset).expand(raw.z, raw.y, raw.x).clone()
    filled = torch.zeros_like(want, dtype=torch.bool)
    for zz in (-1, 0, 1):
        for yy in (-1, 0, 1):
            for xx in (-1, 0, 1):
                sel = (dz == zz) & (dy == yy) & (dx == xx)
                if (xx, yy, zz) == (0, 0, 0) or radius.dir(xx, yy, zz) != 0:
                    filled |= sel
    if boundary is not None:
        # nothing crosses a non-periodic face of the global grid: cells outside it keep their poison
        for axis, (g, n) in enumerate(((gx, X), (gy, Y), (gz, Z))):
            for side in (-1, 1):
                face = [0, 0, 0]
                face[axis] = side
                if not boundary.face_periodic(*face):
                    out = (g < 0) if side < 0 else (g >= n)
                    filled &= ~out.expand_as(filled)
    want[~filled] = poison
    return want


def check_exchange(dd, q: int, radius, poison: int = POISON, boundary=None, offset: int = 0):
    """Return the number of wrong cells over every local sub-domain."""
    bad = 0
    for di in range(dd.num_domains()):
        t = dd.curr(di, q).cpu()
        if t.is_floating_point():
            # NaN poison (race canary) must never survive in a cell that should have been written
            t = torch.nan_to_num(t, nan=float(poison))
        got = t.long()
        want = expected_full(dd, di, radius, poison, boundary, offset)
        bad += int((got != want).sum())
    return bad


# ---- byte-level oracle: any element size, both backends, only the byte API (region_from_host / quantity_to_host) ----
# The coordinate encoding above overflows 1- and 2-byte elements and needs a typed view, which opaque (Bytes)
# quantities do not have. Here every BYTE of a cell is a hash of (global coordinate, quantity, byte index, tag), so a
# copy that moves the wrong half of an element, or the right bytes of another quantity, shows as a wrong cell.

_M64 = (1 << 64) - 1


def cell_bytes(gz, gy, gx, q: int, es: int, tag: int = 0) -> np.ndarray:
    """uint8 array (..., es): byte b of the cell at global (gz, gy, gx) of quantity q is a fixed integer hash of
    (gz, gy, gx, q, b, tag) modulo 251, so a pattern byte is never the 0xFF poison. gz, gy, gx broadcast."""
    gz, gy, gx = np.broadcast_arrays(np.asarray(gz, dtype=np.int64), np.asarray(gy, dtype=np.int64),
                                     np.asarray(gx, dtype=np.int64))
    b = np.arange(es, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = (gz.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + gy.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F)
             + gx.astype(np.uint64) * np.uint64(0x165667B19E3779F9))[..., None]
        h = h + (b + np.uint64(1)) * np.uint64(0xD6E8FEB86659FD93)
        h = h + np.uint64(((q + 1) * 0xA0761D6478BD642F + (tag + 1) * 0xE7037ED1A0B428DB) & _M64)
        # splitmix64 finalizer: every input bit reaches the low bits the modulus keeps
        h ^= h >> np.uint64(30)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(27)
        h *= np.uint64(0x94D049BB133111EB)
        h ^= h >> np.uint64(31)
    return (h % np.uint64(251)).astype(np.uint8)


def _raw_coords(d):
    """global (z, y, x) coordinate arrays of every raw cell (halo included) of local domain d, shaped to broadcast"""
    org, raw = d.accessor_origin(), d.raw_size()
    gz = np.arange(raw.z, dtype=np.int64).reshape(-1, 1, 1) + org.z
    gy = np.arange(raw.y, dtype=np.int64).reshape(1, -1, 1) + org.y
    gx = np.arange(raw.x, dtype=np.int64).reshape(1, 1, -1) + org.x
    return gz, gy, gx


def fill_bytes_pattern(dd, q: int, tag: int = 0):
    """Poison both buffers of quantity q (every byte 0xFF), then write cell_bytes into every sub-domain's interior."""
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        es = d.elem_size(q)
        d.fill_bytes(q, POISON_BYTE, True, True)
        o, s, r = d.origin(), d.size(), d.radius()
        gz = np.arange(s.z, dtype=np.int64).reshape(-1, 1, 1) + o.z
        gy = np.arange(s.y, dtype=np.int64).reshape(1, -1, 1) + o.y
        gx = np.arange(s.x, dtype=np.int64).reshape(1, 1, -1) + o.x
        data = cell_bytes(gz, gy, gx, q, es, tag)
        d.region_from_host(_C.Dim3(r.x(-1), r.y(-1), r.z(-1)), s, q, data.tobytes(), True)


def expected_bytes(dd, di: int, q: int, radius, tag: int = 0) -> np.ndarray:
    """(z, y, x, es) uint8: what the raw cells of sub-domain di hold after one exchange of a fill_bytes_pattern field"""
    d = dd.domain(di)
    es = d.elem_size(q)
    cr = d.get_compute_region()
    Z, Y, X = dd.size().z, dd.size().y, dd.size().x
    gz, gy, gx = _raw_coords(d)
    dz = (gz >= cr.hi.z).astype(np.int64) - (gz < cr.lo.z).astype(np.int64)
    dy = (gy >= cr.hi.y).astype(np.int64) - (gy < cr.lo.y).astype(np.int64)
    dx = (gx >= cr.hi.x).astype(np.int64) - (gx < cr.lo.x).astype(np.int64)
    dz, dy, dx = np.broadcast_arrays(dz, dy, dx)
    want = cell_bytes(gz % Z, gy % Y, gx % X, q, es, tag).copy()
    filled = np.zeros(dz.shape, dtype=bool)
    for zz in (-1, 0, 1):
        for yy in (-1, 0, 1):
            for xx in (-1, 0, 1):
                if (xx, yy, zz) == (0, 0, 0) or radius.dir(xx, yy, zz) != 0:
                    filled |= (dz == zz) & (dy == yy) & (dx == xx)
    want[~filled] = POISON_BYTE
    return want


def check_exchange_bytes(dd, q: int, radius, tag: int = 0) -> int:
    """Number of wrong cells of quantity q over every local sub-domain after exchange(): a cell whose direction class
    has a non-zero radius holds the pattern of its periodic image, every other halo cell is still 0xFF in all its
    bytes, the interior is unchanged. A cell is wrong if any of its bytes differs."""
    bad = 0
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        want = expected_bytes(dd, di, q, radius, tag)
        got = np.frombuffer(d.quantity_to_host(q), dtype=np.uint8)
        assert got.size == want.size, f"quantity_to_host returned {got.size} B, expected {want.size}"
        bad += int((got.reshape(want.shape) != want).any(axis=-1).sum())
    return bad
