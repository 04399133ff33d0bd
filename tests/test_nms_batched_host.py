"""CPU: the batched rotated-NMS entry points of the C ABI — exported, bound, their workspace query consistent with the single
form's, and their argument checks answered before anything touches the device (null device pointers, no GPU needed)."""
import ctypes

import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
NAMES = ("hvpr_nms_bev_batched_workspace_bytes", "hvpr_nms_bev_batched_f32", "hvpr_gather_predictions_batched_f32")


@pytest.fixture(scope="module")
def L():
    from hvpr_amd import build, _lib
    build.build()
    return _lib.lib()


def test_status_codes_are_the_ones_named_here(L):
    assert L.hvpr_status_string(OK) == b"ok"
    assert L.hvpr_status_string(INVALID).startswith(b"invalid")
    assert L.hvpr_status_string(UNSUPPORTED).startswith(b"unsupported")
    assert b"workspace" in L.hvpr_status_string(WORKSPACE)


def test_entry_points_exported_and_bound(L):
    from hvpr_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), f"{n} not exported"
        assert n in _lib.SIGNATURES
        assert getattr(L, n).argtypes == _lib.SIGNATURES[n][1]
    assert L.hvpr_abi_version() == 8                         # additive change


def test_workspace_query(L):
    q, single = L.hvpr_nms_bev_batched_workspace_bytes, L.hvpr_nms_workspace_bytes
    ns = (1, 64, 65, 4096, 4097)
    for n in ns:
        assert q(0, n) == 0
        assert q(1, n) == single(n) > 0
    for S in (1, 2, 3, 16, 48):
        assert q(S, 0) == 0
        for n in ns:
            assert q(S, n) >= S * q(1, n)
            assert q(S, n) <= S * (q(1, n) + 255)            # S private copies, each padded to 256 bytes at the most
    # non-decreasing in S and in n
    for n in ns:
        sizes = [q(S, n) for S in range(0, 20)]
        assert sizes == sorted(sizes)
    for S in (1, 2, 16):
        sizes = [q(S, n) for n in (0, 1, 63, 64, 65, 128, 129, 1000, 4095, 4096, 4097, 8192, 16384)]
        assert sizes == sorted(sizes)


def _nms(L, boxes=1, box_stride=7, table_stride=0, spt=1, order=None, n_device=None, S=1, n_max=10, thresh=0.1, max_keep=5,
         mto=1, keep=1, keep_count=1, ws=1, ws_bytes=None, stream=None):
    """Call with fake (never dereferenced) non-null pointers where `1` is given: every case below must return before a launch."""
    p = lambda v: ctypes.c_void_p(0x1000) if v == 1 else None
    if ws_bytes is None:
        ws_bytes = L.hvpr_nms_bev_batched_workspace_bytes(max(S, 0), max(n_max, 0))
    return L.hvpr_nms_bev_batched_f32(p(boxes), box_stride, table_stride, spt, p(order), p(n_device), S, n_max, thresh, max_keep, mto,
                                      p(keep), p(keep_count), p(ws), ws_bytes, stream)


def test_nms_argument_checks_run_before_the_device(L):
    assert _nms(L, S=0) == OK                                # nothing to do, no launch
    assert _nms(L, S=0, boxes=None, keep=None, keep_count=None, ws=None) == OK
    assert _nms(L, S=-1) == INVALID
    assert _nms(L, spt=0) == INVALID
    assert _nms(L, spt=-3) == INVALID
    assert _nms(L, box_stride=6) == INVALID
    assert _nms(L, n_max=-1) == INVALID
    assert _nms(L, max_keep=-1) == INVALID
    assert _nms(L, S=3, boxes=None) == INVALID
    assert _nms(L, S=3, keep=None) == INVALID
    assert _nms(L, S=3, keep_count=None) == INVALID
    assert _nms(L, S=3, n_max=0, keep_count=None) == INVALID  # the counts are what n_max == 0 writes
    assert _nms(L, S=3, ws=None) == INVALID
    assert _nms(L, S=2, n_max=16385) == UNSUPPORTED
    for S, n in ((1, 10), (4, 700), (2, 4096), (2, 4160)):
        need = L.hvpr_nms_bev_batched_workspace_bytes(S, n)
        assert _nms(L, S=S, n_max=n, ws_bytes=need - 1) == WORKSPACE
        assert _nms(L, S=S, n_max=n, ws_bytes=0) == WORKSPACE
    # a workspace made for S - 1 segments does not serve S
    assert _nms(L, S=4, n_max=700, ws_bytes=L.hvpr_nms_bev_batched_workspace_bytes(3, 700)) == WORKSPACE


def test_single_form_keeps_its_checks(L):
    p = ctypes.c_void_p(0x1000)
    f = L.hvpr_nms_bev_f32
    assert f(p, 6, None, None, 10, 0.1, 5, 1, p, p, p, 1 << 30, None) == INVALID
    assert f(p, 7, None, None, -1, 0.1, 5, 1, p, p, p, 1 << 30, None) == INVALID
    assert f(p, 7, None, None, 10, 0.1, 5, 1, p, None, p, 1 << 30, None) == INVALID
    assert f(None, 7, None, None, 10, 0.1, 5, 1, p, p, p, 1 << 30, None) == INVALID
    assert f(p, 7, None, None, 16385, 0.1, 5, 1, p, p, p, 1 << 30, None) == UNSUPPORTED
    assert f(p, 7, None, None, 4096, 0.1, 5, 1, p, p, p, L.hvpr_nms_workspace_bytes(4096) - 1, None) == WORKSPACE


def test_gather_argument_checks_run_before_the_device(L):
    p = ctypes.c_void_p(0x1000)
    g = L.hvpr_gather_predictions_batched_f32
    good = [p, 7, 700, 1, p, p, 100, p, 2, 5, p, p, p, p, None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[{"boxes": 0, "box_stride": 1, "spt": 3, "scores": 4, "labels": 5, "keep": 7, "S": 8, "K": 9, "ob": 10, "os": 11, "ol": 12,
               "osel": 13}[k]] = v
        return g(*a)
    assert call(S=0) == OK
    assert call(K=0) == OK
    assert call(S=-1) == INVALID
    assert call(K=-1) == INVALID
    assert call(spt=0) == INVALID
    assert call(box_stride=6) == INVALID
    for k in ("boxes", "scores", "labels", "keep", "ob", "os", "ol", "osel"):
        assert call(**{k: None}) == INVALID, k
