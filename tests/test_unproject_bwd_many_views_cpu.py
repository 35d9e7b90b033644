"""lt_unproject_bwd with more than 8 camera views, without a GPU: the view limit and the workspace size (argument validation runs before any device
work, so dummy non-null pointers are enough)."""
import ctypes

import pytest

import lt_hip as H

ERR_INVALID, ERR_UNSUPPORTED = -1, -2          # LT_ERR_INVALID, LT_ERR_UNSUPPORTED


@pytest.fixture(autouse=True)
def _gather_path(monkeypatch):
    monkeypatch.delenv("LT_UNPROJ_BWD_ATOMICS", raising=False)


def _call(NV, C=32, workspace=None, nbytes=0):
    one = ctypes.c_void_p(16)
    l = H.lib()
    rc = l.lt_unproject_bwd(H.LT_F32, one, one, one, None, one, one, None, 2, NV, C, 24, 24, 16, 16, 16, H.AGG["softmax"], workspace, nbytes, None)
    return rc, l.lt_last_error().decode()


@pytest.mark.parametrize("NV", [9, 32])
def test_more_than_eight_views_pass_the_view_check_and_stop_at_the_missing_workspace(NV):
    rc, msg = _call(NV)
    assert rc == ERR_INVALID, (rc, msg)
    assert "workspace" in msg, msg
    # one byte short of one sample's share is refused the same way, and the message names the share
    per_sample = H.lib().lt_unproject_bwd_workspace(1, NV, 32, 16, 16, 16)
    rc, msg = _call(NV, workspace=ctypes.c_void_p(256), nbytes=per_sample - 1)
    assert rc == ERR_INVALID and "workspace of at least %d bytes" % per_sample in msg, (rc, msg)


def test_eight_views_and_fewer_are_checked_as_before():
    for NV in (1, 4, 8):
        rc, msg = _call(NV)
        assert rc == ERR_INVALID and "workspace" in msg, (NV, rc, msg)
    rc, msg = _call(0)
    assert rc == ERR_UNSUPPORTED and "NV=0" in msg, (rc, msg)


def test_the_view_limit_is_32_and_the_message_names_it():
    rc, msg = _call(33)
    assert rc == ERR_UNSUPPORTED, (rc, msg)
    assert "NV <= 32" in msg and "NV=33" in msg, msg


def test_workspace_is_the_sum_of_its_five_aligned_blocks():
    def a256(v):
        return (v + 255) // 256 * 256

    B, NV, C, V = 1, 31, 32, 64
    nvox, nbricks = V ** 3, (V // 4) ** 3
    nblk1 = min(2048, (nvox * (C // 4) + 255) // 256)
    want = a256(NV * nvox * C * 4) + a256(NV * nbricks * 16) + a256(nblk1 * NV * C * 8) + a256(NV * nvox * 4) + a256(NV * nvox * 16)
    l = H.lib()
    assert l.lt_unproject_bwd_workspace(B, NV, C, V, V, V) == want
    assert a256(NV * nvox * C * 4) == 1040187392          # the dxs block: 1.04 GB per sample at CMU's 31 views
    assert l.lt_unproject_bwd_workspace(3, NV, C, V, V, V) == 3 * want
    # ragged grid: bricks round up
    want2 = a256(9 * 210 * 16 * 4) + a256(9 * 2 * 2 * 2 * 16) + a256(4 * 9 * 16 * 8) + a256(9 * 210 * 4) + a256(9 * 210 * 16)
    assert l.lt_unproject_bwd_workspace(1, 9, 16, 5, 6, 7) == want2
