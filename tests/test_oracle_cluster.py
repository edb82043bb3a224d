"""Pin the cluster-path oracle: fixture parity + agreement with the real reference TUs."""
import os

import numpy as np
import pytest

from rattle_amd import synth


def test_oracle_reproduces_toyset_clusters_fixture(oracle, toyset, toyset_clusters):
    """`cluster --rna` (k=10, defaults) on the recovered toyset == toyset/rna/output/clusters.out:
    546 clusters, every member, member order, representative and strand."""
    seqs = [r[1] for r in toyset]                      # already length-descending, ids = positions
    got, counters = oracle.cluster_reads(seqs, k=10, is_rna=True)
    want = [((m[0], m[1], -1), [(s[0], s[1], -1) for s in seqs_]) for m, seqs_ in toyset_clusters]
    assert len(got) == 546
    assert got == want
    assert counters[0] > 9_000_000 and counters[1] > 300_000       # SURVEY section 6 work profile


def test_restatement_matches_reference_units(oracle, ref_lib):
    """k-mer lists, bit-vectors, intersection, LIS and var vs kmer.cpp/similarity.cpp/utils.cpp."""
    seqs, _, tid, _ = synth.reads(60, 6, 2, True, seed=11)
    for k in (6, 10, 11, 16):
        for s in seqs[:8]:
            a = oracle.extract_kmers(s, k, True)
            b = ref_lib.extract_kmers(s, k, True)
            assert len(a) == len(b) and [ref_lib.digest(x) for x in a] == list(b)
    n = 0
    for i in range(0, 40):
        for j in range(i + 1, min(i + 6, 60)):
            for strand in (0, 1):
                for k in (10, 11):
                    a = oracle.pair_score(seqs[i], seqs[j], k, strand)
                    b = ref_lib.pair_score(seqs[i], seqs[j], k, strand)
                    assert a[0] == b[0] and a[2] == b[2] and a[4] == b[4]
                    if a[4] > 0:
                        assert a[1] == b[1]
                    assert ref_lib.digest(a[5]) == b[5]
                    assert a[3] == b[3] or (np.isnan(a[3]) and np.isnan(b[3]))
                    n += 1
    assert n > 500
    # repeats: cross product on equal hashes (kmer.cpp:56-61)
    lowc = b"ACACACACACACACACACACACACACACACAC" * 6 + b"GGTTA" * 10
    a = oracle.pair_score(lowc, lowc[7:] + b"ACGT", 6, 0)
    b = ref_lib.pair_score(lowc, lowc[7:] + b"ACGT", 6, 0)
    assert a[:3] == b[:3] and a[4] == b[4] and a[4] > 2000


def test_var_edge_cases(oracle, ref_lib):
    assert oracle.var([]) == 0.0 and ref_lib.var([]) == 0.0
    assert np.isnan(oracle.var([5])) and np.isnan(ref_lib.var([5]))        # 0/0, utils.cpp:54
    rng = np.random.default_rng(5)
    for n in (2, 3, 17, 400):
        v = rng.integers(-60, 60, n)
        assert oracle.var(v) == ref_lib.var(v)


def test_restated_readers_match_the_real_fasta_cpp(oracle, ref_lib, tmp_path):
    """The four readers of fasta.cpp (FASTQ / FASTA x plain / cluster variant: labels appended to headers, running record
    index, length filter, N skip, upper-casing of FASTA, DOS line ends) as restated in oracle/orc_io.hpp, record for record
    against the real translation unit in oracle/_ref (or its recorded answers, tests/conftest.py RefAnswers)."""
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "oracle_cli")
    fq = b"@a 1\nACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIII\n@b\nACGTNACGT\n+x\n#########\n@c\nACG\n+\n!!!\n@d extra words\nacgtACGTacgtACGTacgt\n+\nJJJJJJJJJJJJJJJJJJJJ\n"
    fa = b">s1 first\nACGTACGTAC\nGTACGTAC\n\n>s2\nacgtnacgt\n>s3\nACG\n>s4\nacgtacgtacgtacgtacgt\nACGT\n"
    files = {"u.fq": fq, "d.fq": fq.replace(b"\n", b"\r\n"), "u.fa": fa, "d.fa": fa.replace(b"\n", b"\r\n")}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    for name in files:
        for cluster_variant in (0, 1):
            kind = (2 if name.endswith(".fa") else 0) + cluster_variant
            for label, index, raw, lower in ((b"", 0, 0, 5), (b",lab1", 7, 0, 5), (b",x", 3, 1, 5), (b"", 0, 0, 19)):
                got = tmp_path / "got.txt"
                want, nxt = ref_lib.dump_reads(str(tmp_path / name), label, kind, index, raw, lower, 1000)
                args = [cli, "dump-reads", "-i", str(tmp_path / name), "--kind", str(kind), "--index", str(index), "--lower-length", str(lower),
                        "--upper-length", "1000", "-o", str(got)] + (["-l", label.decode()] if label else []) + (["--raw"] if raw else [])
                r = subprocess.run(args, capture_output=True, text=True, check=True)
                assert got.read_bytes() == want, (name, kind, label, index, raw, lower)
                if cluster_variant and want:
                    assert int(r.stdout.strip()) == nxt, (name, kind, label, index, raw, lower)
