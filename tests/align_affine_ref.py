"""The contract of `align_pairs_scored` and `align_cigars_scored` (include/rattle_hip.h) in plain Python, twice, on top of
tests/align_ref.py and tests/cigar_ref.py, and the cases aimed at the three-state kernels.

Gotoh's local alignment with a scoring (m, x, o, e) of four positive magnitudes: match +m, mismatch -x, the first gapped column of a gap
-o, every further one -e (spoa's convention: 8,6 is `correct`'s engine, 8,8 is linear); 1 <= m, x <= 64, 1 <= e <= o <= 64.  With i over
the read (reverse-complemented first on strand 1), j over the transcript, letters A, C, G, T = U:

  U[i][j] = max(H[i-1][j] - o, U[i-1][j] - e)     a read base against a gap        U[0][*] = -inf
  L[i][j] = max(H[i][j-1] - o, L[i][j-1] - e)     a transcript base against a gap  L[*][0] = -inf
  H[i][j] = max(0, H[i-1][j-1] + s(q_i, t_j), U[i][j], L[i][j])                    H[0][*] = H[*][0] = 0

A cell with H == 0 begins a new alignment.  In H ties go diagonal, then U, then L; in U and in L open wins a tie with extend; the end cell
is the largest H, ties to the smallest i, then the smallest j.

Fact 1.  H >= U and H >= L on every cell (H is the maximum of a set that holds both).  A gap state on a path is positive: the gap ends
in a cell whose positive H equals its gap state, and every step back along the gap adds e or o.  So every cell a path visits in a gap
state has H >= U > 0 (H >= L > 0): no path runs through a cell whose H is 0, in any state, and since a gap state is entered only from
an H and left only into an H it equals, the first and the last column of every alignment are diagonal.

Fact 2.  With o == e, U[i][j] = max(H[i-1][j], U[i-1][j]) - o = H[i-1][j] - o by fact 1, open wins every tie, and so the path is cell
for cell the linear path of align_ref with gap -o.

The recurrence itself is written once, in tests/align_model.py; the names below are its functions at the mode LOCAL:

  fill(q, t, sc)        the three matrices
  walk(q, t, F, i, j)   from the end cell back: the cells of the path (end first) and the (cell, state) pairs it visits
  traceback(q, t, sc)   the classic form: fill, end cell, walk, count the columns
  forward(q, t, sc)     what the kernel does: every state of every cell carries (start_i, start_j, matches, mismatches) of the path the
                        rule picks for it; a gap step copies the payload of the state it comes from, a diagonal step out of a zero
                        cell starts at the cell's own coordinates; q_gap = sq - M - X, t_gap = st - M - X from the two spans
  full / rectangle      record and ops from the whole matrices / from the rectangle of the record alone (cigar_ref's pair of forms)

No device, no numpy in the recurrences."""
import numpy as np

import align_model as M
import align_ref as R
import cigar_ref as CG

NEG, H_, U_, L_ = M.NEG, M.H_, M.U_, M.L_           # minus infinity, and the states of a walk
LINEAR, ENGINE, MM2, LONG = (5, 4, 8, 8), (5, 4, 8, 6), (2, 4, 4, 2), (5, 4, 12, 1)
SCORINGS = (LINEAR, ENGINE, MM2, LONG)

# the model at this mode, under the signatures of the list above; walk(..., open_wins=False) is the opposite tie rule in a gap state,
# records(..., max_cells=0, form="full") and cigars(..., max_cells=0) are what the _scored calls return for a case, pair(q, t, rev, sc)
# is (record on the read as given, ops) of one pair, remembered
check_scoring = M.check_scoring
fill, walk, full, forward, rectangle, pair, records, cigars = M.bind(M.LOCAL, "fill", "walk", "full", "forward", "rectangle", "pair", "records", "cigars")


def traceback(q: bytes, t: bytes, sc):
    return full(q, t, sc)[0]


# ---- cases for the three-state kernels: (targets, reads, target_of_read, rev) --------------------------------------------------------
def exon_pair(seed=5, flank=60, insert=40):
    """the pair of the README: two random flanks, a random insert in the transcript only"""
    rng = np.random.default_rng(seed)
    f1, x, f2 = R.rnd(rng, flank), R.rnd(rng, insert), R.rnd(rng, flank)
    return f1 + f2, f1 + x + f2


def gap_case(seed=31):
    """Exons that one sequence lacks, between 60-base flanks: a 40- and a 70-base insert in the read (one I run) and in the transcript
    (one D run).  Read side, rows counted from 0: the 70-base run behind a front flank cut to 50 bases lies in rows 50 - 119, the
    40-base run in rows 60 - 99 and a 10-base run in rows 60 - 69, so each crosses the block edge at row 64 in U, through the strip.
    (A 70-base gap costs 8 + 69 * 6 = 422 under 8,6, more than a 60-base flank earns, so only 12,1 spans it; 40 bases cost 242.)
    Then the four long-gap pairs again with 70 random bases in front of both sequences, so that the rectangle does not begin at 0:
    kernel F's blocks, counted from the rectangle's first row, are then not kernel E's."""
    rng = np.random.default_rng(seed)
    pairs = []
    f = [R.rnd(rng, 60) for _ in range(4)]
    x40, x70, x10 = R.rnd(rng, 40), R.rnd(rng, 70), R.rnd(rng, 10)
    pairs.append((f[0][10:] + x70 + f[1], f[0][10:] + f[1], 0))          # [0] I run in rows 50 - 119
    pairs.append((f[2] + x10 + f[3], f[2] + f[3], 0))                    # [1] I run in rows 60 - 69
    pairs.append((f[0] + x40 + f[1], f[0] + f[1], 0))                    # [2] I run in rows 60 - 99
    pairs.append((f[0] + f[1], f[0] + x40 + f[1], 0))                    # [3], [4] D runs of 40 and 70
    pairs.append((f[2] + f[3], f[2] + x70 + f[3], 0))
    for q, t, _ in list(pairs[:1]) + list(pairs[2:5]):
        pairs.append((R.rnd(rng, 70) + q, R.rnd(rng, 70) + t, 0))
    return R.pairs_case(pairs)


def block_edge_case(seed=32):
    """A gap that ends in row 64 exactly (its last I row is the last row of block 0, DP row 64), one that begins there (its first I row
    is DP row 65, lane 0 of block 1 -- its open comes through the strip), a 130-column D run across two refills, and a 150-row I run
    that crosses two block edges in U."""
    rng = np.random.default_rng(seed)
    a, b, c = R.rnd(rng, 60), R.rnd(rng, 64), R.rnd(rng, 70)
    g4, g12, g130, g150 = R.rnd(rng, 4), R.rnd(rng, 12), R.rnd(rng, 130), R.rnd(rng, 150)
    return R.pairs_case([(a + g4 + c, a + c, 0),            # I rows (1-based) 61 - 64
                         (b + g12 + c, b + c, 0),           # I rows 65 - 76
                         (a + c, a + g130 + c, 0),          # D columns 61 - 190
                         (a[:40] + g150 + c, a[:40] + c, 0)])      # I rows 41 - 190: blocks 0, 1 and 2


def homopolymer_case():
    """homopolymers and repeats of unequal length: under o = 2 e (8,4; 4,2) a gap of two columns ties with two gaps of one"""
    rng = np.random.default_rng(33)
    a, b = R.rnd(rng, 30), R.rnd(rng, 30)
    return R.pairs_case([(b"A" * 40, b"A" * 47, 0), (b"A" * 47, b"A" * 40, 0), (a + b"G" * 7 + b, a + b"G" * 10 + b, 0),
                         (a + b"G" * 10 + b, a + b"G" * 7 + b, 0), (a + b"GA" * 8 + b, a + b"AG" * 10 + b, 0),
                         (b"A" * 70 + a, b"A" * 66 + a, 0)])


CASES = {"gaps": gap_case, "block_edges": block_edge_case, "homopolymers": homopolymer_case}
EDGE_CASES = ("gaps", "block_edges", "homopolymers", "ties", "zero_crossing", "status")      # run under every scoring; the others under two


def all_cases():
    """name -> builder: align_ref's, cigar_ref's and the ones above"""
    return {**R.CASES, **CG.CASES, **CASES}
