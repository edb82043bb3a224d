"""Cases and measuring helpers aimed at what the cases of tests/align_ref.py, cigar_ref.py, align_affine_ref.py and align_ends_ref.py leave
unpinned in kernels E and F (csrc/pair_align.hip, csrc/pair_cigar.hip): the order of the end cell across lanes, blocks and refills, the
co-optimal choices (diagonal, up, left; open before extend) beyond the first block edge, the reverse strand at every edge length and at
chosen q_start, pairs of sixteen and more row blocks, and scorings at both ends of the accepted range.

The references stay as they are.  What is added here measures the CASES, on the CPU: walks of the reference matrices under a WRONG rule
(tests/align_model.py's walk with H order "udl" or "dlu" for the rule's "dul", extend before open), an end cell keyed the wrong way round, and the path cells on which two
choices tie, by row and by column.  A case pins a rule where the wrong rule changes its CIGAR; tests/test_align_sweep.py asserts that it
does, and where.  `mode` is "local" (align_affine_ref's matrices) or "read" (align_ends_ref's) throughout.

Builders return (targets, reads, target_of_read, rev); no case hands a reference more than 2e6 cells.  No device, no numpy in the walks."""
import numpy as np

import align_affine_ref as A
import align_ends_ref as E
import align_model as M
import align_ref as R
import cigar_ref as CG
from align_model import fill, walk                  # fill(q, t, sc, mode); walk(q, t, F, i, j, sc, mode, order="dul", open_wins=True)

MODES = M.MODES                                     # "local" and "read"
# both ends of every magnitude; x > 2 o with o > e (1,64,64,1 has it the other way: a gap never pays); x > 2 o with o == e (1,64,1,1;
# 2,5,2,2); o == e other than 8 (those two, 1,1,1,1, 64,64,64,64 and 3,2,5,5): by fact 2 of align_affine_ref the linear path
SWEEP_SCORINGS = ((1, 1, 1, 1), (64, 64, 64, 64), (64, 1, 64, 1), (64, 64, 64, 1), (1, 64, 64, 1), (1, 64, 1, 1), (2, 5, 2, 2), (3, 2, 5, 5))
CHEAP_GAPS = ((1, 64, 1, 1), (2, 5, 2, 2))          # a mismatch costs more than a gap in each sequence: "up before left" decides often


def scoring_id(sc) -> str:
    return "linear" if sc is None else ".".join(map(str, sc))


# ---- the model by mode, and what a wrong rule changes ----------------------------------------------------------------------------------
def ref(mode):
    """the module that states the contract of `mode` and binds the model at it"""
    return {"local": A, "read": E}[mode]


def records(case, sc, mode, **kw):
    return M.records(*case, sc, mode, **kw)


def cigars(case, sc, mode, **kw):
    return M.cigars(*case, sc, mode, **kw)


def submitted(case):
    """[(index, read on the strand aligned, transcript)] of the pairs a kernel sees"""
    targets, reads, tor, rev = case
    return [(r, R.revcomp(q) if s else q, targets[x]) for r, (q, x, s) in enumerate(zip(reads, tor, rev)) if x >= 0 and q and targets[x]]


def end_cell(F, mode):
    """the rule's end cell (score, i, j); None where nothing aligns locally"""
    end = M.end_cell(F, mode)
    return end if mode == "read" or end[0] > 0 else None


def end_cell_ji(F, mode):
    """The end cell keyed the wrong way round.  Local: the largest H, ties to the smallest j, then the smallest i (a lane reduction keyed
    (score, j, i)).  Read: the last row has one i, so the wrong key there is the LARGEST j (a `>=` for the `>`)."""
    H = F[0]
    if mode == "read":
        row = H[-1]
        best = max(row[1:])
        return best, len(H) - 1, max(j for j in range(1, len(row)) if row[j] == best)
    best = max(max(row) for row in H)
    if best <= 0:
        return None
    j, i = min((j, i) for i, row in enumerate(H) for j, h in enumerate(row) if h == best)
    return best, i, j


def tie_cells(q, t, F, visits, sc):
    """The visits of a walk at which the rule had a choice: [(i, j, kind)], kind "h" where two or three of diagonal, U and L reproduce H,
    "g" where open ties with extend in the gap state the walk is in.  Same for both modes (a visit lies in row and column >= 1)."""
    m, x, o, e = sc
    H, U, L = F
    q, t = q.translate(R._T), t.translate(R._T)
    out = []
    for i, j, state in visits:
        if state == A.H_:
            h = H[i][j]
            n = (h == H[i - 1][j - 1] + (m if q[i - 1] == t[j - 1] else -x)) + (h == U[i][j]) + (h == L[i][j])
            if n >= 2:
                out.append((i, j, "h"))
        else:
            M, di, dj = (U, 1, 0) if state == A.U_ else (L, 0, 1)
            if H[i - di][j - dj] - o == M[i - di][j - dj] - e:
                out.append((i, j, "g"))
    return out


def count_ties(ties, kind=None, row=0, col=0):
    """how many of tie_cells' cells are of `kind` (None: either) and lie beyond DP row `row` and beyond DP column `col`"""
    return sum(1 for i, j, k in ties if (kind is None or k == kind) and i > row and j > col)


def full(q, t, sc, mode):
    """One pair on the strand aligned, from the whole matrices, by the model's fill, end cell and walk: (record, ops, visits, matrices).
    (align_ref.NONE, [], [], F) where nothing aligns locally."""
    F = fill(q, t, sc, mode)
    return M.record(q, t, F, sc, mode) + (F,)


def gap_held_two_steps(visits) -> bool:
    """does a walk stay in a gap state for two steps in a row?  (With o == e it never does: open wins every tie, fact 2.)"""
    return any(a[2] != A.H_ and a[2] == b[2] for a, b in zip(visits, visits[1:]))


def wrong_rule(case, sc, mode, order="dul", open_wins=True, row=64):
    """What a wrong rule changes in a case: (pairs whose CIGAR it changes, those of them whose two paths differ in a cell beyond DP row
    `row` -- beyond the first block edge of kernel E, and of kernel F wherever the rectangle begins in row 0 --, [tie_cells of the rule's
    path, per aligned pair])."""
    changed = beyond = 0
    ties = []
    for r, q, t in submitted(case):
        F = fill(q, t, sc, mode)
        end = end_cell(F, mode)
        if end is None:
            continue
        _, i, j = end
        path, visits = walk(q, t, F, i, j, sc, mode)
        ties.append(tie_cells(q, t, F, visits, sc))
        other, _ = walk(q, t, F, i, j, sc, mode, order, open_wins)
        if CG.ops_of_path(q, t, other) != CG.ops_of_path(q, t, path):
            changed += 1
            beyond += any(a > row for a, _ in set(path) ^ set(other))
    return changed, beyond, ties


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
END_ORDER_JUNK = ((20, 20), (50, 70), (109, 30), (30, 109), (130, 130))
END_ORDER_LOCAL = range(0, 10)                      # two end cells tie locally: (20, Lt) wins over (Lq, 20)
END_ORDER_READ = range(10, 12)                      # three end columns tie in the last row: 20 wins over 90 and 170
END_ORDER_COLUMNS = (20, 90, 170)


def end_order_case(seed=51):
    """Pairs 0 - 4: the read x + J1 + y on the transcript y + J2 + x, |x| = |y| = 20, J1 of A and C, J2 of G and T (nothing bridges), with
    (|J1|, |J2|) of END_ORDER_JUNK.  x on x ends in cell (20, Lt), y on y in (Lq, 20), both with 20 matches: the rule takes the smaller i.
    With |J1| = 30 the loser's row 70 is lane 5 of block 1, below the winner's lane 19; with 109 and 130 the two cells are two blocks and
    two refills apart.  Pairs 5 - 9: the same transposed (the read y + J2 + x on x + J1 + y).  Pairs 10, 11: the read x, on either strand,
    on x + J + x + J' + x with |J| = 50, |J'| = 60: the last row ties in columns 20, 90 and 170, three refills; the smallest j wins."""
    rng = np.random.default_rng(seed)
    x, y = R.rnd(rng, 20), R.rnd(rng, 20)
    pairs = []
    for n1, n2 in END_ORDER_JUNK:
        pairs.append((x + CG._junk(rng, n1, b"AC") + y, y + CG._junk(rng, n2, b"GT") + x, 0))
    pairs += [(t, q, 0) for q, t, _ in list(pairs)]
    t = x + R.rnd(rng, 50) + x + R.rnd(rng, 60) + x
    pairs += [(x, t, 0), (R.revcomp(x).replace(b"T", b"U"), t, 1)]
    return R.pairs_case(pairs)


SHIFTS = (24, 57, 60, 63, 64, 88, 121, 127, 128)
SHIFT_PARTS = ((24, 57, 60, 63, 64), (88, 121), (127, 128))          # each part below 2e6 cells for a reference


def shifted_tie_case(shifts=SHIFTS, seed=52):
    """Every pair of align_ref.tie_cases and align_affine_ref.homopolymer_case behind a common random prefix of each length of `shifts`
    on both sequences: the prefix aligns, and the repeats' co-optimal choices then lie on and around rows and columns 64 and 128 -- where
    kernel E's payload and kernel F's U bit come through the strip, a refill and a new window.  12 pairs per shift."""
    rng = np.random.default_rng(seed)
    base = [(q, targets[x]) for targets, reads, tor, _ in (R.tie_cases(), A.homopolymer_case()) for q, x in zip(reads, tor)]
    pairs = []
    for n in shifts:
        for q, t in base:
            p = R.rnd(rng, n)
            pairs.append((p + q, p + t, 0))
    return R.pairs_case(pairs)


STRAND_SPANS = (1, 63, 64, 65, 127, 128, 129)
STRAND_FLANKS = ((0, 0), (1, 64), (65, 3))          # bases before and after the span on the transcript's strand: q_start is the second


def strand_edge_case(seed=53):
    """Strand 1, the reads written with U.  On the transcript's strand the read is f1 + span' + f2 with (|f1|, |f2|) of STRAND_FLANKS and
    the transcript g1 + span + g2 with (|g1|, |g2|) = (|f2|, |f1|); span' is the span with a substitution every 20 bases, none within 8
    of an end, no indel; the read's flanks are of A and C and the transcript's of G and T, so no cell outside the span's rectangle has a
    match behind or in front of it and the local alignment is the span exactly: q_end - q_start is the span's length, every length of
    STRAND_SPANS, and q_start (on the read as given) is |f2| = 0, 64 and 3.  (The one-base span is an A between flanks of C alone: its
    only match.)  Pairs 0 - 20.  Pairs 21 - 34: the pairs with flanks again on the span alone as the transcript, which is shorter than the
    read: in read mode the flanks are overhang runs, computed on the reverse strand."""
    rng = np.random.default_rng(seed)
    pairs, short = [], []
    for n in STRAND_SPANS:
        for n1, n2 in STRAND_FLANKS:
            span = R.rnd(rng, n) if n > 1 else b"A"
            copy = bytearray(span)
            for k in range(10, n - 8, 20):
                copy[k] = b"ACGT"[(b"ACGT".index(copy[k]) + 1 + k // 20 % 3) % 4]
            mine = b"C" if n == 1 else b"AC"
            fwd = CG._junk(rng, n1, mine) + bytes(copy) + CG._junk(rng, n2, mine)
            q = R.revcomp(fwd).replace(b"T", b"U")
            pairs.append((q, CG._junk(rng, n2, b"GT") + span + CG._junk(rng, n1, b"GT"), 1))
            if n1 + n2:
                short.append((q, span, 1))
    return R.pairs_case(pairs + short)


def many_blocks_pairs(seed=54):
    """(read as sequenced, transcript, read on the transcript's strand): a transcript of 1080 bases and a read of about 1110, 70 unrelated
    bases in front of a copy of the transcript's bases 20 - 1060 with 6 % errors.  (A local alignment of 1024 rows needs as many columns,
    less its gaps: the transcript cannot be much shorter than the read.)"""
    rng = np.random.default_rng(seed)
    t = R.rnd(rng, 1080)
    fwd = R.rnd(rng, 70) + R.mutate(rng, t[20:1060], 0.06)
    return R.revcomp(fwd).replace(b"T", b"U"), t, fwd


def many_blocks_case(transposed=False):
    """One pair of 18 row blocks and 17 refills, about 1.2e6 cells: the read of many_blocks_pairs on strand 1, or (transposed) the
    transcript as the read on strand 0 -- 17 blocks, 18 refills.  Either aligns locally over more than 1024 rows: kernel E's strip is
    rewritten in place 17 times, and kernel F's records lie in 16 and more rows of b (cols + 63)."""
    q, t, fwd = many_blocks_pairs()
    return R.pairs_case([(t, fwd, 0)] if transposed else [(q, t, 1)])


CASES = {"end_order": end_order_case, "strand_edges": strand_edge_case, "many_blocks": many_blocks_case,
         "many_blocks_t": lambda: many_blocks_case(True),
         **{f"shifted_{k}": (lambda part=part: shifted_tie_case(part)) for k, part in enumerate(SHIFT_PARTS)}}
SHIFTED = tuple(f"shifted_{k}" for k in range(len(SHIFT_PARTS)))
# the cases of the three references that run under every SWEEP_SCORINGS entry beside SHIFTED and "strand_edges"
SWEPT_OLD = ("ties", "homopolymers", "zero_crossing", "status", "block_edges", "gaps", "edges", "ends_edges", "overhangs", "strand", "random")
SWEPT = SWEPT_OLD + SHIFTED + ("strand_edges",)


def all_cases():
    """name -> builder: those of the four references, and the ones above"""
    return {**E.all_cases(), **CASES}
