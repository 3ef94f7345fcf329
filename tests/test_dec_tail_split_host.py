"""CPU: dlsg_dec_tail_split, the split dlsg_dec_tail_fwd chooses for a sampled step's vocabulary scan (host only, no launch), and
the defines that go with it as dlsg_amd.abi reads them from include/dlsg.h."""
import pytest

from dlsg_amd import abi, hip


@pytest.mark.parametrize('B, cus, want', [(64, 256, 4), (128, 256, 2), (129, 256, 1), (256, 256, 1), (640, 256, 1),
                                          (1, 256, 8),        # capped at DLSG_DEC_TAIL_MAX_SPLIT
                                          (300, 256, 1),      # more rows than compute units
                                          (32, 256, 8), (33, 256, 7), (64, 304, 4), (64, 0, 1)])
def test_split_is_cus_over_rows_capped(B, cus, want):
    lib = hip.load_library()
    assert lib.dlsg_dec_tail_split(B, cus) == want == max(1, min(abi.defines['DLSG_DEC_TAIL_MAX_SPLIT'], cus // B))


def test_defines_and_fields_are_visible():
    assert abi.defines['DLSG_DEC_TAIL_MAX_SPLIT'] == 8
    # a row of the workspace holds one 8-byte pair per part and the ticket counter
    assert abi.defines['DLSG_DEC_TAIL_WS_WORDS'] >= 2 * abi.defines['DLSG_DEC_TAIL_MAX_SPLIT'] + 1
    names = [n for n, _ in abi.structs['dlsg_dec_tail_args']._fields_]
    assert names[-3:-1] == ['s_ws', 's_split']          # appended: a zeroed struct of the earlier layout means the unsplit launch
    a = abi.structs['dlsg_dec_tail_args']()
    assert not a.s_ws and a.s_split == 0
