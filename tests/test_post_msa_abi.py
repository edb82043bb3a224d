"""The test hook rattle_hip_debug_post_msa at the edges that need no device: its input is checked on the host before anything
is uploaded (kernel D scatters every base to the column it is given), so on a host context a bad input is an argument error and
a good one stops at the missing device."""
import numpy as np
import pytest

from rattle_amd._lib import RattleError
from rattle_amd.api import Context, msa_pack

ROWS = [b"ACGT-ACGTA", b"AC-TTACGTA", b"ACGTTAC-TA"]
QUALS = [bytes([60] * (10 - r.count(b"-"))) for r in ROWS]


@pytest.fixture(scope="module")
def host_ctx():
    ctx = Context(None)
    yield ctx
    ctx.close()


def refused(ctx, packs, mode, code, text):
    with pytest.raises(RattleError) as e:
        ctx.debug_post_msa(packs, mode)
    assert f"error {code}:" in str(e.value) and text in str(e.value), str(e.value)


def test_a_good_msa_reaches_the_device_check(host_ctx):
    refused(host_ctx, [msa_pack(ROWS, QUALS)], 1, -3, "no device")
    refused(host_ctx, [msa_pack(ROWS)], 2, -3, "no device")
    # a pack of width 0 is what a skipped pack looks like: its columns are not looked at
    refused(host_ctx, [(0, [b"ACG", b"T"], [np.array([7, 7, 1], np.uint32), np.array([99], np.uint32)], None)], 2, -3, "no device")


@pytest.mark.parametrize("mode", [0, 3, -1])
def test_a_mode_other_than_1_or_2_is_refused(host_ctx, mode):
    refused(host_ctx, [msa_pack(ROWS, QUALS)], mode, -2, "mode must be 1")


def test_mode_1_without_qualities_is_refused(host_ctx):
    refused(host_ctx, [msa_pack(ROWS)], 1, -2, "needs the qualities")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("cols, text", [([0, 1, 2, 2], "not strictly increasing"), ([0, 2, 1, 3], "not strictly increasing"),
                                        ([0, 1, 2, 10], "not below the pack's width"), ([6, 7, 8, 2 ** 32 - 1], "not below the pack's width")])
def test_bad_columns_are_refused(host_ctx, mode, cols, text):
    width, seqs, columns, quals = msa_pack(ROWS, QUALS)
    seqs[1], columns[1], quals[1] = b"ACGT", np.array(cols, np.uint32), b"<<<<"
    refused(host_ctx, [msa_pack(ROWS, QUALS), (width, seqs, columns, quals)], mode, -2, text)


def test_a_base_outside_the_alphabet_is_refused(host_ctx):
    width, seqs, columns, quals = msa_pack(ROWS, QUALS)
    seqs[2] = b"ACGNTACTA"
    refused(host_ctx, [(width, seqs, columns, quals)], 1, -2, "a base other than")
    seqs[2] = b"ACG-TACTA"
    refused(host_ctx, [(width, seqs, columns, quals)], 1, -2, "a base other than")
