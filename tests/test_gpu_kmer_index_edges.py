"""Kernel K (kmer_extract.hip) at every size class, pass count and lane edge, against oracle.extract_kmers through
rattle_hip_load_reads / rattle_hip_get_read_index.  Bit-exact: hashes, positions, the 4096-bit 6-mer vectors and their popcount.

build_index sorts the reads into classes by padded list length P = 64 .. 8192 (sorted in LDS) and >= 16384 (the bitonic network in
global scratch); the list lengths here sit one below, on and one above every class edge, so that each class runs with a full list and
with one of a single k-mer more than half.  P = 8192 needs more than 64 KB of dynamic LDS in both kernels (the radix kernel's
shm2 = 512 + Lmax + 4096 + 64 + 12 P is about 111 KB, the bitonic kernel's 512 + Lmax + 8 P about 74 KB): the hipFuncSetAttribute
branches.  nk = 8192 is also the last length whose positions fit the radix kernel's 16-bit values."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NK = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193,
      16383, 16384, 16385)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _read_set(k):
    """per list length: random ACGT; a homopolymer (all 64 lanes of a step hold one digit and move one cursor, and equal hashes
    must stay in position order across the wavefronts' quarters); period 2 (two digits, two hashes).  In shuffled order, so that
    the classes interleave in d_items."""
    rng = np.random.default_rng(4000 + k)
    reads = []
    for i, nk in enumerate(NK):
        L = nk + k
        reads += [ACGT[rng.integers(0, 4, L)].tobytes(), b"ACGT"[i % 4:i % 4 + 1] * L, (b"AC" * L)[:L]]
    if k == 16:
        reads += [b"ACGTACG", b"ACGTACGTTGCAGGAT", b"ACGTACGTTGCAGGATC"]       # L = 7: nk = 0 but one 6-mer; L = k; L = k + 1
    return [reads[i] for i in rng.permutation(len(reads))]


def _check(gpu_ctx, oracle, reads, k, both):
    gpu_ctx.load_reads(reads, k, both)
    for r, s in enumerate(reads):
        fh, fp, rh, rp, bf, br = oracle.extract_kmers(s, k, both)
        h, p, bv, pc = gpu_ctx.read_index(r, 0)
        label = (k, r, len(s), s[:4])
        assert np.array_equal(h, fh) and np.array_equal(p, fp), ("forward list", label)
        assert np.array_equal(bv, bf), ("forward vector", label)
        assert pc == int(np.bitwise_count(bf).sum()), ("popcount", label)
        if both:
            h, p, bv, _ = gpu_ctx.read_index(r, 1)
            assert np.array_equal(h, rh) and np.array_equal(p, rp), ("reverse list", label)
            assert np.array_equal(bv, br), ("reverse vector", label)


@pytest.mark.parametrize("k", [1, 4, 5, 8, 10, 11, 12, 13, 16])
def test_radix_sort_every_class_and_pass_count(gpu_ctx, oracle, k, monkeypatch):
    """kmer_extract_lsd_kernel for P = 64 .. 8192, kmer_extract_kernel with global scratch beyond.  `for (shift = 0; shift < 2 * k;
    shift += 8)` makes ceil(2k / 8) passes -- 1 for k = 1, 4; 2 for 5, 8; 3 for 10, 11, 12; 4 for 13, 16 -- and the sorted list is in
    `ka` after the last swap, whichever of the two buffers that is; 2k is a multiple of 8 (k = 4, 8, 12, 16) or the last digit is
    short.  A wavefront's quarter `seg = (nk + 255) / 256 * 64`: nk = 1, 63, 64 leave three quarters empty (`s0 = s1 = nk`), 65 and
    129 end a quarter one key into a 64-key step (`valid = i < s1`), 127, 255, 511 .. one key short of it, 128, 256, 512 .. exactly
    on it.  nk = 0 (L = k, and L = 7 < k with one 6-mer) writes no list and still the vector."""
    monkeypatch.delenv("RATTLE_KMER_SORT", raising=False)
    _check(gpu_ctx, oracle, _read_set(k), k, True)


@pytest.mark.parametrize("k", [5, 11, 16])
def test_bitonic_sort_every_class(gpu_ctx, oracle, k, monkeypatch):
    """RATTLE_KMER_SORT=bitonic: kmer_extract_kernel's `bitonic_sort_lds` for every class up to P = 8192 (`shm > 64 * 1024`: the
    LDS opt-in of the bitonic kernel), the padding keys ~0 behind lists that are no power of two, `bitonic_sort_global` beyond."""
    monkeypatch.setenv("RATTLE_KMER_SORT", "bitonic")
    _check(gpu_ctx, oracle, _read_set(k), k, True)


def test_forward_only_index(gpu_ctx, oracle, monkeypatch):
    """`dim3(m, ns)` with ns = 1: no reverse-strand block, kh[1] / kp[1] / bv[1] never reserved"""
    monkeypatch.delenv("RATTLE_KMER_SORT", raising=False)
    _check(gpu_ctx, oracle, _read_set(11), 11, False)
