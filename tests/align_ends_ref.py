"""The contract of the READ mode of `align_pairs_mode` and `align_cigars_mode` (include/rattle_hip.h, RATTLE_ALIGN_READ) in plain Python,
twice, on top of tests/align_ref.py, tests/cigar_ref.py and tests/align_affine_ref.py, and the cases aimed at what the mode changes in
kernels E and F.

The read is aligned from its first base to its last, the transcript's ends are free (semi-global).  Scoring (m, x, o, e) as in
align_affine_ref; the linear form is 5,4,8,8.  With i over the read (reverse-complemented first on strand 1), j over the transcript:

  H[0][j] = 0 for j = 0..Lt          U[0][*] = -inf        (the alignment may begin at any transcript position)
  H[i][0] = U[i][0] = -(o + (i-1) e) L[*][0] = -inf        (read bases before the transcript's first base: a gap)
  U[i][j] = max(H[i-1][j] - o, U[i-1][j] - e)
  L[i][j] = max(H[i][j-1] - o, L[i][j-1] - e)
  H[i][j] = max(H[i-1][j-1] + s(q_i, t_j), U[i][j], L[i][j])           -- no zero floor

Ties as in align_affine_ref: in H diagonal, then U, then L; in U and L open wins a tie with extend.  The end cell is the largest
H[Lq][j] over j = 1..Lt, ties to the smallest j.  The walk goes back to row 0 and ends in (0, t_start); row 0 has no left moves, and a
walk that reaches column 0 goes straight up: the remaining rows are one I run.  The record has status 0, q_start = 0, q_end = Lq, a
score that may be zero or negative, and t_end - t_start may be 0 (the whole read one I run).

The recurrence itself is written once, in tests/align_model.py; the names below are its functions at the mode READ:

  fill(q, t, sc)        the three matrices
  walk(q, t, F, j, sc)  from H[Lq][j] back to row 0: the cells of the path (end first) and the (cell, state) pairs it visits
  full(q, t, sc)        fill, end cell, walk, count the columns: (record, ops)
  forward(q, t, sc)     what kernel E does: every state of every cell carries (start_j, matches, mismatches) of its path; row 0 starts
                        a path at its own column, column 0 at column 0
  rectangle(...)        what kernel F does: the same recurrence over columns (t_start, t_end] alone, with this mode's borders

No device, no numpy in the recurrences."""
import numpy as np

import align_affine_ref as A
import align_model as M
import align_ref as R
import cigar_ref as CG

NEG = A.NEG
H_, U_, L_ = A.H_, A.U_, A.L_
CHEAP_GAP = (1, 64, 1, 1)                           # a mismatch costs more than any short gap: t_end == t_start occurs
SCORINGS = A.SCORINGS + (CHEAP_GAP,)

# the model at this mode, under the signatures of the list above; records(..., max_cells=0, form="full") and cigars(..., max_cells=0) are
# what the _mode calls return for a case in read mode, pair(q, t, rev, sc) is (record on the read as given, ops) of one pair, remembered
fill, full, forward, rectangle, pair, records, cigars = M.bind(M.READ, "fill", "full", "forward", "rectangle", "pair", "records", "cigars")
border = lambda i, sc: M.border(i, sc, M.READ)[0]                           # H[i][0] = U[i][0], i >= 1
end_cell = lambda H: M.end_cell((H,), M.READ)[::2]                          # (score, j) of the last row
walk = lambda q, t, F, j, sc: M.walk(q, t, F, len(q), j, sc, M.READ)        # from H[Lq][j]


# ---- cases for the read mode: (targets, reads, target_of_read, rev) -------------------------------------------------------------------
OVERHANGS = (1, 5, 63, 64, 65, 70)


def overhang_case(seed=41):
    """The read runs 1, 5, 63, 64, 65 and 70 bases past the transcript's start (pairs 0 - 5), past its end (6 - 11) and past both
    (12 - 17); the transcript is 120 random bases.  A leading overhang of n bases is an I run in rows 1 - n of column 0, the border: the
    70-base one crosses the block edge at row 64 there, the 65-base one ends in row 65, lane 0 of block 1.  A trailing one is an I run in
    the last n rows, in the transcript's last column."""
    rng = np.random.default_rng(seed)
    t = R.rnd(rng, 120)
    pairs = [(R.rnd(rng, n) + t[:100], t, 0) for n in OVERHANGS]
    pairs += [(t[20:] + R.rnd(rng, n), t, 0) for n in OVERHANGS]
    pairs += [(R.rnd(rng, n) + t + R.rnd(rng, n), t, 0) for n in OVERHANGS]
    return R.pairs_case(pairs)


def foreign_exon_parts(seed=42):
    """(A, X, B): two first exons of 40 bases that share no letter (A of A and C, X of G and T), and a common rest of 120"""
    rng = np.random.default_rng(seed)
    return CG._junk(rng, 40, b"AC"), CG._junk(rng, 40, b"GT"), R.rnd(rng, 120)


def foreign_exon_case():
    """The README's example: transcripts A+B and X+B, the read A+B on each.  Locally the read on X+B is 120= with q_start 40; in read mode
    its first 40 bases are on the line, and AS is lower than on A+B by what they cost."""
    a, x, b = foreign_exon_parts()
    return [a + b, x + b], [a + b, a + b], [0, 1], [0, 0]


EDGES = (1, 63, 64, 65, 127, 128, 129)
# the named pairs of ends_edge_case, behind the 49 crossed lengths
E_UNRELATED, E_ZERO_SCORE, E_ZERO_MID, E_TIE, E_NO_COLUMN, E_NO_COLUMN_LONG, E_ONE_ONE, E_ONE_ONE_X, E_ONE_ROW, E_ONE_COL, E_STRAND = range(49, 60)


def ends_edge_case(seed=43):
    """Reads of 1, 63 - 65, 127 - 129 bases against transcripts of the same lengths, crossed, pieces of one ancestor (pairs 0 - 48: every
    block and refill edge of both kernels, with overhangs wherever the read is the longer one); then
      49  unrelated sequences: a negative score
      50  4 matches and 5 mismatches: the score is exactly 0 under 5,4,*,*
      51  the same in front of 60 matches: H == 0 in the middle of the chosen path, passed through
      52  AAAA on A * 10: every end column from 4 on ties, t_end = 4 and t_start = 0
      53  CC on AA: under 1,64,1,1 the read is one I run, t_end == t_start
      54  70 C on 5 A: the same across a block edge
      55 - 58  Lq = 1 and Lt = 1, equal and unequal; one row; one column
      59  strand 1, the read written with U"""
    rng = np.random.default_rng(seed)
    base = R.rnd(rng, 160)
    pairs = []
    for lq in EDGES:
        for lt in EDGES:
            q, t = R.mutate(rng, base, 0.1), R.mutate(rng, base, 0.05)
            pairs.append(((q + R.rnd(rng, lq))[:lq], (t + R.rnd(rng, lt))[:lt], 0))
    tail = R.rnd(rng, 60)
    t = R.rnd(rng, 90)
    q = R.rnd(rng, 7) + R.mutate(rng, t[10:80], 0.08) + R.rnd(rng, 4)
    pairs += [(CG._junk(rng, 50, b"AC"), CG._junk(rng, 60, b"GT"), 0),
              (b"ACGTAAAAA", b"ACGTCCCCC", 0),
              (b"ACGTAAAAA" + tail, b"ACGTCCCCC" + tail, 0),
              (b"AAAA", b"A" * 10, 0),
              (b"CC", b"AA", 0),
              (b"C" * 70, b"A" * 5, 0),
              (b"A", b"A", 0), (b"A", b"C", 0), (b"G", R.rnd(rng, 10), 0), (R.rnd(rng, 10), b"G", 0),
              (R.revcomp(q).replace(b"T", b"U"), t, 1)]
    return R.pairs_case(pairs)


CASES = {"overhangs": overhang_case, "foreign_exon": foreign_exon_case, "ends_edges": ends_edge_case}
EDGE_CASES = A.EDGE_CASES + tuple(CASES)            # run under every scoring; the others under two


def all_cases():
    """name -> builder: those of the three references below, and the ones above"""
    return {**A.all_cases(), **CASES}
