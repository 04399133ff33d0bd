"""CPU: hvpr_attend_rows_fwd_f32 is exported and bound, and every argument check is answered on the host — none of these calls may
touch a device, so they run on a machine without one (the pointers are dummies that are never dereferenced)."""
import ctypes

import pytest

NAME = "hvpr_attend_rows_fwd_f32"
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def L():
    from hvpr_amd import _lib, build
    build.build()
    return _lib.lib()


def test_symbol_is_exported_and_bound(L):
    from hvpr_amd import _lib
    assert NAME in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert L.hvpr_status_string(INVALID_ARG) == b"invalid argument" and L.hvpr_status_string(UNSUPPORTED).startswith(b"unsupported")
    assert L.hvpr_abi_version() == 8                       # 8: the float-atomic scatters are gone, no signature changed


def test_python_wrapper_has_no_cpu_fallback():
    import torch
    from hvpr_amd import kernels
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.attend_rows(torch.zeros(4, 64), torch.zeros(100, 64), torch.zeros(4, 20, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.attend_rows(torch.zeros(4, 64), torch.zeros(80, 64), None, 20)


def test_argument_checks_are_made_on_the_host(L):
    buf = (ctypes.c_float * 64)()                          # one dummy non-null address for every pointer
    p = ctypes.addressof(buf)
    fn = getattr(L, NAME)

    def call(q=p, M=4, rows=p, N=100, idx=p, k=20, C=64, out=p, w=p):
        return fn(q, M, rows, N, idx, k, C, out, w, None)

    assert call(C=32) == UNSUPPORTED
    assert call(k=0) == UNSUPPORTED
    assert call(k=33) == UNSUPPORTED
    assert call(out=None) == INVALID_ARG
    assert call(M=0) == OK
    # the rest of the documented contract
    assert call(q=None) == INVALID_ARG and call(rows=None) == INVALID_ARG and call(w=None) == INVALID_ARG
    assert call(M=-1) == INVALID_ARG and call(N=-1) == INVALID_ARG and call(k=-1) == INVALID_ARG
    assert call(idx=None, N=79) == INVALID_ARG            # dense form: N must be M * k
    assert call(M=0, q=None, rows=None, idx=None, out=None, w=None, N=0) == OK
