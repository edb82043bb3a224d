"""Packs whose letters are not one four-letter alphabet: T beside U, bytes that are no base at all, five letters in one column.

Kernel C (poa.hip) scores a pack of {A,C,G,T} or of {A,C,G,U} from a table indexed by (c >> 1) & 3, where T and U -- and every byte of
ALIAS below and its letter -- share an index; any other pack compares letters byte by byte, and it may turn into such a pack after any
of its sequences.  No GPU and no oracle in here: tests/test_constructed_alphabets.py proves on the oracle that every pack sits where its
name says (above all that its MSA changes when every byte is replaced by its table twin, so a kernel that took the table where it must
compare gives other rows), tests/test_gpu_poa_alphabet.py runs the same packs through every form of the row loop.

Every builder works at four lengths, one per packed column class (LENGTHS); a pack is 6 to 8 noisy copies of one random transcript with
6 % noise (substitutions, insertions and deletions at 2 % each, drawn from the read's own alphabet) and a 5' truncation of up to 30
bases: deep and noisy enough for bubbles, ties and far predecessors.  Everything is deterministic from the builder's arguments; BUMP
moves the seed of a pack whose draw does not pass its proof."""
import numpy as np

LENGTHS = (600, 1100, 1600, 2100)            # the longest read of a pack in column classes 0 .. 3 (CPL 4, 6, 8, 10), about
DEPTH = 8
ACGT = np.frombuffer(b"ACGT", np.uint8)
ACGU = np.frombuffer(b"ACGU", np.uint8)
# by table index (c >> 1) & 3: the letter and the bytes the table would score as a match with it
ALIAS = (b"A@a\x80", b"CBc", b"TUt", b"GFgN")
ALIAS_ALL = np.frombuffer(b"".join(ALIAS), np.uint8)
ORDERS = ("interleaved", "u_first", "t_first")
WHERE = ("second", "middle", "last")
BUMP = {}                                    # pack name -> added to its seed

_TWIN = bytes(b"ACTG"[(c >> 1) & 3] for c in range(256))
_T, _U = ord("T"), ord("U")


def twin(pack):
    """every byte replaced by the letter of its table index: what a kernel that took the table for this pack would align"""
    return [s.translate(_TWIN) for s in pack]


def _rng(kind, cls, variant=0, name=None):
    return np.random.default_rng([20261019, kind, cls, variant, BUMP.get(name, 0)])


def _noisy(rng, tx, abc, err=0.06):
    """substitutions, deletions and insertions at err / 3 each, the new letters from abc"""
    r = rng.random(len(tx))
    s = tx.copy()
    sub = (r >= err / 3) & (r < 2 * err / 3)
    s[sub] = abc[rng.integers(0, len(abc), int(sub.sum()))]
    s = s[r >= err / 3]
    pos = np.sort(rng.integers(0, len(s) + 1, int(err / 3 * len(s))))
    return np.insert(s, pos, abc[rng.integers(0, len(abc), len(pos))])


def _with_u(a):
    return np.where(a == _T, _U, a).astype(np.uint8)


def _copies(rng, tx, written):
    """one noisy copy of tx per entry of `written` ("U": T written as U, noise from ACGU; "T": as it is, noise from ACGT); the first
    read whole, the others 5'-truncated by up to 30 bases"""
    pack = []
    for k, w in enumerate(written):
        s = _noisy(rng, _with_u(tx), ACGU) if w == "U" else _noisy(rng, tx, ACGT)
        pack.append(s[0 if k == 0 else int(rng.integers(0, 30)):].tobytes())
    return pack


def strands(cls, order, depth=DEPTH):
    """Half of the reads written with U; the other half noisy copies of the same transcript written with T, which is how a member marked
    `rev` looks after the reference's complement (U -> A, A -> T).  order: "interleaved" (U, T, U, ...), "u_first", "t_first"."""
    rng = _rng(1, cls, ORDERS.index(order), "strands/%s/%d" % (order, cls))
    tx = ACGT[rng.integers(0, 4, LENGTHS[cls])]
    h = depth // 2
    written = {"interleaved": "UT" * h, "u_first": "U" * h + "T" * h, "t_first": "T" * h + "U" * h}[order]
    return _copies(rng, tx, written)


def late_m(where, depth=DEPTH):
    return {"second": 1, "middle": depth // 2, "last": depth - 1}[where]


def late(cls, where, depth=DEPTH):
    """Reads 0 .. m - 1 in ACGT only, read m the first with U (then U and T in turn): the table serves the first alignments, the compare
    path the rest.  where: "second" (m = 1), "middle", "last"."""
    rng = _rng(2, cls, WHERE.index(where), "late/%s/%d" % (where, cls))
    tx = ACGT[rng.integers(0, 4, LENGTHS[cls])]
    m = late_m(where, depth)
    return _copies(rng, tx, "T" * m + ("UT" * depth)[:depth - m])


def alias(cls, depth=DEPTH, rewrite=0.15):
    """A transcript in ACGT; every read rewrites 15 % of its bases as a byte of the same table index (ALIAS: `@`, `a` and 0x80 with A, `B`
    and `c` with C, `U` and `t` with T, `F`, `g` and `N` with G) and draws its noise from the whole set."""
    rng = _rng(3, cls, 0, "alias/%d" % cls)
    tx = ACGT[rng.integers(0, 4, LENGTHS[cls])]
    sets = [np.frombuffer(a, np.uint8) for a in ALIAS]
    pack = []
    for k in range(depth):
        s = _noisy(rng, tx, ALIAS_ALL)
        hit = np.nonzero(rng.random(len(s)) < rewrite)[0]
        for i in hit:
            a = sets[(int(s[i]) >> 1) & 3]
            s[i] = a[rng.integers(0, len(a))]
        pack.append(s[0 if k == 0 else int(rng.integers(0, 30)):].tobytes())
    return pack


# the letters of reads 0 .. 4 at the four constructed columns of five(): U arrives last, first, second and in the middle
FIVE_ORDERS = (b"ACGTU", b"UTGCA", b"GUACT", b"TAUCG")


def five_columns(cls):
    """two adjacent columns, and two on their own, all far from the ends (the alignment is local: a lone mismatch at an end is clipped)"""
    L = LENGTHS[cls]
    return [L // 3, L // 3 + 1, L // 2, 2 * L // 3 + 5]


def five(cls):
    """Seven reads, identical except at the columns of five_columns, where reads 0 .. 4 hold A, C, G, T and U in the orders of FIVE_ORDERS:
    an aligned group of five nodes per column (n_al = 4, the most the group record holds), built in another order every time.  Reads 5 and 6
    are reads 0 and 3 again: two alignments against the finished groups.  Returns (pack, columns)."""
    rng = _rng(4, cls, 0, "five/%d" % cls)
    B = ACGT[rng.integers(0, 4, LENGTHS[cls])].copy()
    cols = five_columns(cls)
    reads = []
    for i in range(5):
        r = B.copy()
        for c, order in zip(cols, FIVE_ORDERS):
            r[c] = order[i]
        reads.append(r.tobytes())
    return reads + [reads[0], reads[3]], cols


def six():
    """five(0) without its copies, and a sixth read with N at the third constructed column: one letter more than an aligned group holds.
    Returns (pack, column)."""
    pack, cols = five(0)
    r = bytearray(pack[0])
    r[cols[2]] = ord("N")
    return pack[:5] + [bytes(r)], cols[2]


NEAR_SHAPES = ("late", "strands")
POA_BAND_SPREAD = 400


def near(cls, shape):
    """For the band: 3 to 5 near-identical reads (0.3 % substitutions, 5'-truncated by less than 300 < POA_BAND_SPREAD), the longest of
    LENGTHS[cls].  shape "late": U arrives with the last read, so the earlier alignments can have a certified band; "strands": U and T in
    turn from the first read on."""
    rng = _rng(5, cls, NEAR_SHAPES.index(shape), "near/%s/%d" % (shape, cls))
    depth = (3, 4, 5, 4)[cls]
    tx = ACGT[rng.integers(0, 4, LENGTHS[cls])]
    pack = []
    for k in range(depth):
        s = tx[0 if k == 0 else int(rng.integers(0, 300)):].copy()
        hit = rng.random(len(s)) < (0.003 if k else 0.0)
        s[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        u = k == depth - 1 if shape == "late" else k % 2 == 0
        pack.append((_with_u(s) if u else s).tobytes())
    return pack


def class4():
    """one shallow `strands` pack of class 4 (2561 .. 4096 columns, the wide rows): a U read and a T read of one transcript of 3000 nt"""
    rng = _rng(6, 4, 0, "class4")
    tx = ACGT[rng.integers(0, 4, 3000)]
    return _copies(rng, tx, "UT")


def twin_packs():
    """name -> pack: everything whose MSA must change under twin()"""
    out = {}
    for cls in range(4):
        for order in ORDERS:
            out["strands/%s/%d" % (order, cls)] = strands(cls, order)
        for where in WHERE:
            out["late/%s/%d" % (where, cls)] = late(cls, where)
        out["alias/%d" % cls] = alias(cls)
    return out


def form_packs():
    """name -> pack: what tests/test_gpu_poa_alphabet.py sends through every form of the row loop (the last character of a name is the
    pack's column class)"""
    out = twin_packs()
    for cls in range(4):
        out["five/%d" % cls] = five(cls)[0]
    return out
