"""Named, seeded cases of vigo_update_grid_region: a byte grid and a list of updates (lo, box bytes, r or None) applied in
turn.  tests/test_grid_update_core.py holds the host twin and the core header's word functions against `model` below (the
rule of include/vigo.h restated in numpy over gate_cases.dilate_reference); tests/test_gpu_grid_update.py holds the device
against the host twin on the same cases."""
from dataclasses import dataclass, field

import numpy as np

from gate_cases import dilate_reference

GRIDS = [(6, 5, 70), (5, 4, 33), (4, 4, 32), (9, 7, 41), (1, 6, 40), (40, 24, 70)]
RADII = [(0, 0, 0), (1, 1, 1), (2, 3, 1), (0, 0, 31), (4, 5, 6), (50, 3, 2)]   # the last two: larger than the box / than an axis


@dataclass
class Update:
    lo: tuple
    box: np.ndarray          # uint8 [n0, n1, n2]; an extent may be 0
    r: object = None         # None: raw mode, else (rx, ry, rz)


@dataclass
class Case:
    name: str
    vox: np.ndarray          # uint8 [nx, ny, nz], bits 0..2
    updates: list = field(default_factory=list)


def model(vox, u):
    """the grid after one update, by the rule: raw = the box' bytes assigned; inflate = bits 1.. assigned, then bit 0 of the
    box grown by r := the r-dilation of the whole new occupied plane"""
    out = vox.copy()
    n = u.box.shape
    if 0 in n:
        return out
    sl = tuple(slice(l, l + k) for l, k in zip(u.lo, n))
    if u.r is None:
        out[sl] = u.box
        return out
    out[sl] = (u.box & ~np.uint8(1)) | (out[sl] & 1)
    dil = dilate_reference(((out >> 2) & 1).astype(bool), u.r)
    g = tuple(slice(max(l - rr, 0), min(l + k + rr, d)) for l, k, rr, d in zip(u.lo, n, u.r, vox.shape))
    out[g] = (out[g] & ~np.uint8(1)) | dil[g].astype(np.uint8)
    return out


def expected(case):
    """the byte grid after each update of the case"""
    grids, cur = [], case.vox
    for u in case.updates:
        cur = model(cur, u)
        grids.append(cur)
    return grids


def random_bytes(rng, shape, p_occ=0.04):
    occ = rng.random(shape) < p_occ
    unk = rng.random(shape) < 0.2
    inf = rng.random(shape) < 0.3
    return (inf.astype(np.uint8) | (unk.astype(np.uint8) << 1) | (occ.astype(np.uint8) << 2)).astype(np.uint8)


def inflated(vox, r):
    """the grid with bit 0 := the r-dilation of bit 2 (what vigo_inflate_grid leaves)"""
    dil = dilate_reference(((vox >> 2) & 1).astype(bool), r)
    return ((vox & ~np.uint8(1)) | dil.astype(np.uint8)).astype(np.uint8)


def _families(dims):
    """(name, lo, n) of the box families that fit the grid"""
    nx, ny, nz = dims
    x0, y0 = min(1, nx - 1), min(1, ny - 1)
    n01 = (max(1, min(3, nx - x0)), max(1, min(2, ny - y0)))
    fam = [("one_word", (x0, y0, 5), n01 + (3,))]
    if nz >= 34:
        fam.append(("word_edge", (x0, y0, 30), n01 + (4,)))
    if nz > 66:
        fam.append(("three_words", (x0, y0, 20), n01 + (nz - 22,)))
    fam.append(("z_first", (0, 0, 0), (nx, 1, 2)))
    fam.append(("z_last", (x0, y0, nz - 3), n01 + (3,)))
    fam.append(("z_all", (x0, 0, 0), (1, ny, nz)))
    for cx in sorted({0, nx - 1}):
        for cy in sorted({0, ny - 1}):
            for cz in (0, nz - 1):
                fam.append((f"corner_{cx}_{cy}_{cz}", (cx, cy, cz), (1, 1, 1)))
    fam.append(("whole", (0, 0, 0), dims))
    fam.append(("nz_zero", (x0, y0, 7), n01 + (0,)))
    return fam


def family_cases():
    """every grid x box family: one raw update, then one inflate update per radius, each with fresh bytes"""
    cases = []
    for gi, dims in enumerate(GRIDS):
        big = dims[0] * dims[1] * dims[2] > 20000
        fams = _families(dims)
        if big:   # the large grid: more than one block per launch; one corner is enough there
            fams = [f for f in fams if not f[0].startswith("corner") or f[0] == f"corner_{dims[0] - 1}_{dims[1] - 1}_{dims[2] - 1}"]
        for fi, (fname, lo, n) in enumerate(fams):
            rng = np.random.default_rng(7100 + 100 * gi + fi)
            ups = [Update(lo, random_bytes(rng, n, 0.3))]
            for r in (RADII[1:4] if big else RADII):
                ups.append(Update(lo, random_bytes(rng, n, 0.15), r))
            cases.append(Case(f"{dims[0]}x{dims[1]}x{dims[2]}_{fname}", random_bytes(rng, dims), ups))
    return cases


def removed_obstacle_case():
    """r = (1,1,1) on 9x7x41: the occupied voxel A = (4,3,20) is cleared by a one-voxel box while B = (4,3,22), outside the
    box, stays.  (4,3,21) is within r of both: it keeps bit 0; A's other neighbours, e.g. (4,3,19), lose it."""
    vox = np.zeros((9, 7, 41), dtype=np.uint8)
    vox[4, 3, 20] = 4
    vox[4, 3, 22] = 4
    vox[1, 1, 5] = 2
    r = (1, 1, 1)
    return Case("removed_obstacle", inflated(vox, r), [Update((4, 3, 20), np.zeros((1, 1, 1), dtype=np.uint8), r)])


SEQUENCE_R = (1, 2, 1)


def _random_box(rng, dims):
    lo = [int(rng.integers(0, d)) for d in dims]
    n = [int(rng.integers(1, d - l + 1)) for d, l in zip(dims, lo)]
    return tuple(lo), tuple(n)


def sequence_case():
    """20 seeded random boxes in turn on 40x24x70, raw and inflate mode (one r) mixed; the grid starts r-inflated"""
    rng = np.random.default_rng(7777)
    dims = (40, 24, 70)
    vox = inflated(random_bytes(rng, dims, 0.01), SEQUENCE_R)
    ups = []
    for k in range(20):
        lo, n = _random_box(rng, dims)
        n = tuple(min(v, 12) for v in n[:2]) + (n[2],)
        ups.append(Update(lo, random_bytes(rng, n, 0.02), SEQUENCE_R if rng.random() < 0.5 else None))
    return Case("sequence", vox, ups)


def sweep_cases():
    """40 seeded random (grid <= 12x12x75, box, radii); odd cases start from an r-inflated grid"""
    cases = []
    for k in range(40):
        rng = np.random.default_rng(9000 + k)
        dims = (int(rng.integers(1, 13)), int(rng.integers(1, 13)), int(rng.integers(1, 76)))
        lo, n = _random_box(rng, dims)
        r = (int(rng.integers(0, 5)), int(rng.integers(0, 5)), int(rng.integers(0, 32) if k % 4 == 0 else rng.integers(0, 4)))
        vox = random_bytes(rng, dims, 0.05)
        if k % 2:
            vox = inflated(vox, r)
        ups = [Update(lo, random_bytes(rng, n, 0.1), r)]
        lo2, n2 = _random_box(rng, dims)
        ups.append(Update(lo2, random_bytes(rng, n2, 0.1)))
        cases.append(Case(f"sweep{k:02d}_{dims[0]}x{dims[1]}x{dims[2]}", vox, ups))
    return cases


def all_cases():
    return family_cases() + [removed_obstacle_case(), sequence_case()] + sweep_cases()


# (dims, lo, n, r, expected return code): VIGO_ERR_INVALID_ARG = 1?  the codes are read from the library's header by the tests
ERROR_ARGS = [
    ("negative_lo", (-1, 0, 0), (1, 1, 1), None, "INVALID_ARG"),
    ("negative_n", (0, 0, 0), (1, -1, 1), None, "INVALID_ARG"),
    ("beyond_x", (3, 0, 0), (7, 1, 1), None, "INVALID_ARG"),
    ("beyond_z", (0, 0, 40), (1, 1, 2), None, "INVALID_ARG"),
    ("lo_past_the_grid_empty_box", (0, 8, 0), (1, 0, 1), None, "INVALID_ARG"),
    ("negative_radius", (0, 0, 0), (1, 1, 1), (0, -1, 0), "INVALID_ARG"),
    ("rz_32", (0, 0, 0), (1, 1, 1), (0, 0, 32), "UNSUPPORTED"),
    ("rz_32_beats_empty_box", (0, 0, 0), (1, 0, 1), (0, 0, 32), "UNSUPPORTED"),
]
ERROR_DIMS = (9, 7, 41)
