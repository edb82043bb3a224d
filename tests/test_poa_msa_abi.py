"""rattle_hip_poa_msa at the edges that need no device: a sequence is checked on the host before the device is looked at.  Byte 0 is the
padding of kernel C's rows beyond a sequence (a graph node with that letter would match the padding) and '-' is the gap of the rows the
call returns, so neither can be a letter: a pack that holds one is an argument error on a host context, and a good pack stops at the
missing device.  Such input is never sent to a device, by these tests or by any other."""
import pytest

from rattle_amd._lib import RattleError
from rattle_amd.api import Context

GOOD = [[b"ACGTACGTTTGACA", b"ACGACGTTTGACA"], [b"ACGU", b"", b"acgt@N\x80\xff\x01 ~"], [b"A"]]


@pytest.fixture(scope="module")
def host_ctx():
    ctx = Context(None)
    yield ctx
    ctx.close()


def refused(ctx, packs, code, text):
    with pytest.raises(RattleError) as e:
        ctx.poa_msa(packs)
    assert f"error {code}:" in str(e.value) and text in str(e.value), str(e.value)


def test_a_good_pack_reaches_the_device_check(host_ctx):
    refused(host_ctx, GOOD, -3, "no device")
    refused(host_ctx, [[b"ACGT"]], -3, "no device")


def _with(p, q, at, byte):
    packs = [list(x) for x in GOOD]
    s = packs[p][q]
    packs[p][q] = s[:at] + byte + s[at + 1:]
    return packs


# (pack, sequence in the pack, position, the sequence's index in the call)
PLACES = [(0, 0, 0, 0), (0, 0, 13, 0), (0, 1, 6, 1), (1, 2, 0, 4), (1, 2, 11, 4), (2, 0, 0, 5)]


@pytest.mark.parametrize("p,q,at,index", PLACES)
def test_a_zero_byte_is_refused(host_ctx, p, q, at, index):
    refused(host_ctx, _with(p, q, at, b"\0"), -2, f"sequence {index} holds a zero byte")


@pytest.mark.parametrize("p,q,at,index", PLACES)
def test_a_gap_character_is_refused(host_ctx, p, q, at, index):
    refused(host_ctx, _with(p, q, at, b"-"), -2, f"sequence {index} holds '-'")


def test_the_first_bad_sequence_is_named(host_ctx):
    packs = _with(1, 2, 3, b"-")
    packs[0][1] = b"AC\0T"
    refused(host_ctx, packs, -2, "sequence 1 holds a zero byte")
    refused(host_ctx, [[b"ACGT", b"A-\0"]], -2, "sequence 1 holds a zero byte")
