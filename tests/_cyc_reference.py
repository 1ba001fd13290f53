"""The table of launches of tests/test_gpu_gemm_cyc_exact.py and the plain reference of the block-cyclic trailing update
(csrc/dist.hip: update_args / update_local; csrc/gemm.hip: GemmArgs::cyc).  No GPU, no library: tests/test_cyc_reference.py ties
the reference to the host replay of the enumeration and shows that the table sees three classic mistakes.

The layout is restated by brute force over GLOBAL tiles: member `me` of P owns global tile g iff (g // nbt) % P == me and keeps its
tiles in increasing global order, so `owned(P, me, nbt, T)[l]` is cyc_l2g(l) and `before(...)` is cyc_before -- no closed forms.

A reference is a PLAN: {(local tile row, local tile column): (panel tile row of the A operand, of the B operand)} for the tiles the
launch must write,  C[lr, lc] <- beta C0[lr, lc] + alpha P[a] P[b]^T;  every other local tile must come back bitwise unchanged."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

TILE = 128
GRIDS = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (4, 1), (2, 4)]
NBTS = (1, 2, 4)
TS = (11, 13)            # both ragged against nbt * P; on the wider grids some ranks own nothing of a region (or nothing at all)
AB_PRODUCT = (-1.0, 1.0)  # the pair of potrf_dist
AB_OTHER = (0.5, -1.5)    # a further pair with beta / alpha exact (test_gpu_gemm_exact.AB_EXACT)

# row_lo: first global tile row; [col_lo, col_hi): global tile columns; g0: first global tile row of the panel buffer; kt: tiles of k;
# tri: 1 / 3; occ3; ab: (alpha, beta); opts: context options of the launch
Case = namedtuple("Case", "name row_lo col_lo col_hi g0 kt tri occ3 ab opts")


def owned(P: int, me: int, nbt: int, T: int) -> list[int]:
    return [g for g in range(T) if (g // nbt) % P == me]


def before(P: int, me: int, nbt: int, g: int) -> int:
    return sum(1 for x in range(g) if (x // nbt) % P == me)


def cases(nbt: int, T: int) -> list[Case]:
    """The regions of one factorisation step as potrf_dist states them: panel p = [c0, c1), the next panel q = [c1, q1).  T = 11 takes
    the first panel, T = 13 the second (g0 > 0 either way)."""
    c0 = 0 if T == 11 else nbt
    c1 = c0 + nbt
    q1 = min(T, c1 + nbt)
    kt = c1 - c0
    t_done = c1 + 3                                    # a block append: the new rows start INSIDE a block for nbt = 2, 4
    out = []
    g3 = {"gemm3": 1, "gemm3_fact": 1}                 # the three-workgroup body for the symmetric updates too (with occ3)
    for band in (4, 8, 16):                            # set_option accepts gemm_band (not init-only): launch_impl reads it per launch
        out.append(Case(f"fresh-band{band}", c1, c1, T, c1, kt, 1, 0, AB_PRODUCT, {"gemm3": 0, "gemm_band": band}))
    out.append(Case("fresh-other-scalars", c1, c1, T, c1, kt, 1, 1, AB_OTHER, dict(g3, gemm_band=8)))
    out.append(Case("ahead", c1, c1, q1, c1, kt, 3, 0, AB_PRODUCT, {"gemm3": 0, "gemm_band": 8}))
    out.append(Case("ahead-gemm3", c1, c1, q1, c1, kt, 3, 1, AB_PRODUCT, dict(g3, gemm_band=8)))
    for occ3 in (0, 1):
        for gemm3 in (0, 1):
            for band in (4, 8, 16):
                o = dict(g3, gemm_band=band) if gemm3 else {"gemm3": 0, "gemm_band": band}
                out.append(Case(f"rest-occ{occ3}-gemm3_{gemm3}-band{band}", c1, q1, T, c1, kt, 1, occ3, AB_PRODUCT, o))
    # block append, old panel p: the new rows only, every column right of the panel
    out.append(Case("append", t_done, c1, T, c1, kt, 1, 0, AB_PRODUCT, {"gemm3": 0, "gemm_band": 8}))
    out.append(Case("append-gemm3", t_done, c1, T, c1, kt, 1, 1, AB_PRODUCT, dict(g3, gemm_band=4)))
    # ... and the last old panel, which ends at t_done inside its block: [a0, t_done), 1 .. nbt tiles wide
    a0 = ((t_done - 1) // nbt) * nbt
    out.append(Case("append-last-old-panel", t_done, t_done, T, t_done, t_done - a0, 1, 0, AB_PRODUCT, {"gemm3": 0, "gemm_band": 8}))
    return out


def plan(pr: int, pc: int, my_r: int, my_c: int, nbt: int, T: int, case: Case, wrong: str | None = None) -> dict:
    """{(lr, lc): (a, b)}: local tile (lr, lc) of rank (my_r, my_c), global (gr, gc), is written iff gr >= row_lo, col_lo <= gc < col_hi
    and gr >= gc, from panel tile rows a = gr - g0, b = gc - g0.  wrong: one of the mistakes test_cyc_reference.py wants the table to
    see -- "swap" (my_r and my_c exchanged), "g0" (the panel origin off by one tile), "strict" (gr > gc)."""
    if wrong == "swap":
        my_r, my_c = my_c, my_r
    g0 = case.g0 + (1 if wrong == "g0" else 0)
    rows, cols = owned(pr, my_r, nbt, T), owned(pc, my_c, nbt, T)
    out = {}
    for lr, gr in enumerate(rows):
        for lc, gc in enumerate(cols):
            below = gr > gc if wrong == "strict" else gr >= gc
            if gr >= case.row_lo and case.col_lo <= gc < case.col_hi and below:
                out[(lr, lc)] = (gr - g0, gc - g0)
    return out


def global_tiles(pr: int, pc: int, my_r: int, my_c: int, nbt: int, T: int, pl: dict) -> set:
    rows, cols = owned(pr, my_r, nbt, T), owned(pc, my_c, nbt, T)
    return {(rows[lr], cols[lc]) for lr, lc in pl}


def apply_plan(pl: dict, PPt: np.ndarray, C0: np.ndarray, alpha: float, beta: float) -> np.ndarray:
    """The expected local storage: C0 with the planned tiles replaced by beta C0 + alpha P[a] P[b]^T.  PPt = P P^T on the logical panel
    rows, formed once per panel (integer operands: exact in any order)."""
    ref = C0.copy()
    for (lr, lc), (a, b) in pl.items():
        r, c = slice(lr * TILE, (lr + 1) * TILE), slice(lc * TILE, (lc + 1) * TILE)
        ref[r, c] = beta * C0[r, c] + alpha * PPt[a * TILE:(a + 1) * TILE, b * TILE:(b + 1) * TILE]
    return ref
