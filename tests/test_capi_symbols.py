"""CPU: the C-ABI library builds for gfx950, loads, and exports exactly what include/hvpr_amd.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "hvpr_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hvpr_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def built():
    from hvpr_amd import build
    return build.build()


def test_header_symbols_exported(built):
    L = ctypes.CDLL(built)
    names = _declared()
    assert len(names) >= 8
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/hvpr_amd.h but not exported"


def test_binding_table_matches_header_and_abi_version(built):
    from hvpr_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()
    L = _lib.lib()
    from hvpr_amd import _lib
    assert L.hvpr_abi_version() == _lib.ABI_VERSION == 8
    assert L.hvpr_status_string(0) == b"ok"
    assert L.hvpr_status_string(-2).startswith(b"unsupported")


def test_workspace_queries_need_no_gpu(built):
    from hvpr_amd import _lib
    L = _lib.lib()
    assert L.hvpr_voxelize_workspace_bytes(1, 16384, 296, 248, 1) > 3 * 296 * 248 * 4
    assert L.hvpr_voxelize_workspace_bytes(0, 16384, 296, 248, 1) == 0
    assert L.hvpr_scatter_workspace_bytes(2, 296, 248) == 2 * 296 * 248 * 4


def test_no_cpu_fallback():
    import torch
    from hvpr_amd import kernels
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.memory_readout_fwd(torch.zeros(4, 64), torch.zeros(2000, 64), 20)


# ------------------------------------------------------------------------------------------------ the binding derived from the header
_c = ctypes
_P, _I, _F, _Z, _LL = _c.c_void_p, _c.c_int, _c.c_float, _c.c_size_t, _c.c_longlong
# copied from the hand-typed table the derived one replaced: one of each kind of type (and the plain pillar encoder's, added since)
PINNED = {
    "hvpr_abi_version": (_I, []),
    "hvpr_status_string": (_c.c_char_p, [_I]),
    "hvpr_set_batchnorm_allreduce": (None, [_P, _P]),
    "hvpr_voxelize_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "hvpr_bn_workspace_bytes": (_Z, [_LL, _I]),
    "hvpr_bn_relu_bwd_apply_nhwc_f32": (_I, [_P, _I, _I, _P, _LL, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _c.c_double, _P]),
    "hvpr_fused_sgd_f32": (_I, [_P, _P, _P, _LL, _F, _F, _F, _P, _P]),
    "hvpr_pillar_vfe_plain_fwd_f32": (_I, [_P, _P, _P, _I, _I, _P, _F, _F, _F, _F, _F, _F, _P, _P, _I, _P, _P, _P]),
    "hvpr_kitti_match_f64": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _LL, _P, _I, _I, _P, _I, _P, _I, _P, _P, _I, _I,
                                  _P, _P, _P, _P, _P, _Z, _P]),
    "hvpr_render_bev_u8": (_I, [_P, _LL, _I, _I, _P, _I, _P, _F, _P, _I, _I, _P, _P, _F, _P, _I, _P, _I, _I, _P, _P, _F, _P, _I,
                                _P, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "hvpr_encode_fwd_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _F, _F, _F, _F, _F, _F, _I, _I, _I, _I, _I, _I, _F, _F, _F,
                                 _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P,
                                 _P, _P, _Z, _I, _I, _I, _P]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_derived_signature_equals_the_pinned_one(name):
    from hvpr_amd import _lib
    res, args = _lib.SIGNATURES[name]
    assert (res, list(args)) == PINNED[name]
    assert len(_lib.PARAMS[name]) == len(args)
    assert len(PINNED["hvpr_encode_fwd_f32"][1]) == 52


def test_parameter_kinds_come_from_the_header():
    import torch
    from hvpr_amd import _lib
    kinds = dict(_lib.PARAMS["hvpr_kitti_match_f64"])
    assert len(kinds) == 28                                         # no name twice
    assert kinds["gt_rows"] == torch.float64 and kinds["gt_cls"] == torch.int32 and kinds["gt_dontcare"] == torch.uint8
    assert kinds["gt_off"] == torch.int64 and kinds["workspace"] is _lib.ANY
    assert kinds["n_frames"] is None and kinds["n_gt_total"] is None and kinds["stream"] is None   # scalars (the frame count F)
    assert dict(_lib.PARAMS["hvpr_max_samples_f32"])["G"] is None
    every = [k for ps in _lib.PARAMS.values() for _, k in ps if k is not None]
    # + 8: voxels, num_points, coords, m_device, w, b, pillar_features, pillar_mask of hvpr_pillar_vfe_plain_fwd_f32
    assert len(every) == 569 + 8 == 577 and {k for k in every} == {torch.float32, torch.int32, torch.int64, torch.float64, torch.uint8, _lib.ANY}


def test_parser_on_synthetic_headers():
    import torch
    from hvpr_amd import _lib
    text = """
    /* int in_a_comment(int x); */
    #define NOT_A(x) int macro(int x);
    typedef int (*cb_fn)(double *buf, int n);
    typedef int plain_t;
    int
    broken_over_lines(const int32_t *x,
                      long long n,
                      void *ws);
    size_t sized(void);
    """
    table = _lib.parse_header(text)
    assert sorted(table) == ["broken_over_lines", "sized"]
    res, args, params = table["broken_over_lines"]
    assert res is _I and args == [_P, _LL, _P]
    assert params == (("x", torch.int32), ("n", None), ("ws", _lib.ANY))
    assert table["sized"] == (_Z, [], ())
    for bad in ("int f(unsigned n);", "int f(struct box b);", "int f(const uint16_t *x);", "int f(float *x, bool flag);",
                "unsigned f(int n);", "int f(int);"):
        with pytest.raises(_lib.HvprLibraryError, match=r"f\("):
            _lib.parse_header("size_t ok(int n);\n" + bad)
    # one name declared twice, whatever the two declarations say, raises and is named
    with pytest.raises(_lib.HvprLibraryError, match="again is declared twice"):
        _lib.parse_header("size_t ok(int n);\nint again(const float *x, int n);\nint other(int n);\nsize_t again(void);\n")


def test_missing_header_is_named(tmp_path):
    from hvpr_amd import _lib
    with pytest.raises(_lib.HvprLibraryError, match="nowhere.h"):
        _lib.read_header(str(tmp_path / "nowhere.h"))


def test_call_checks_before_it_reaches_the_library(built):
    import torch
    from hvpr_amd import _lib
    offs = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"hvpr_frame_offsets_f32: points .*no CPU fallback"):
        _lib.call("hvpr_frame_offsets_f32", torch.zeros(3, 5), 3, 5, 1, offs, None)
    with pytest.raises(RuntimeError, match=r"frame_offsets .*no CPU fallback"):     # the second pointer: the first one is NULL
        _lib.call("hvpr_frame_offsets_f32", None, 3, 5, 1, offs, None)
    with pytest.raises(TypeError, match="hvpr_frame_offsets_f32: n_points is a scalar"):
        _lib.call("hvpr_frame_offsets_f32", None, torch.tensor(3), 5, 1, None, None)
    with pytest.raises(TypeError, match="stream is a scalar"):
        _lib.call("hvpr_frame_offsets_f32", None, 3, 5, 1, None, torch.zeros(1))
    with pytest.raises(_lib.HvprLibraryError, match="hvpr_no_such_function"):
        _lib.call("hvpr_no_such_function", 1)
    with pytest.raises(_lib.HvprLibraryError, match="hvpr_voxelize_workspace_bytes"):   # a size query returns no status
        _lib.call("hvpr_voxelize_workspace_bytes", 1, 1, 1, 1, 1)
    # NULL pointers reach the library, whose own argument check answers with its status text
    with pytest.raises(RuntimeError, match="hvpr_frame_offsets_f32 failed"):
        _lib.call("hvpr_frame_offsets_f32", None, 3, 5, 1, None, None)
