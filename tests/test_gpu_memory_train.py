"""hvpr_memory_train_fwd_f32 / _bwd_f32 (csrc/memory_train.hip) against float64, element by element inside the derived rounding bound
of memory_train_cases.py: no tolerance added and no element left out but y, dx and n of the stated near_threshold rows.
test_memory_train_host.py shows on the CPU that an honest fp32 form of the same formulas is inside that bound, that no row of the table
has an item whose support decision the reference cannot take, and that each wrong variant falls outside.  The reference is computed
on the device in float64 from the same fp32 inputs.  Every output lies inside a larger sentinel buffer; every row is run on a zeroed
and on a 0xFF-filled workspace, and twice, and must give the same bits.  Every test reports max(err / bound) under "observed
margins"."""
import pytest
import torch

import memory_train_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # include/hvpr_amd.h hvpr_status
SENTINEL, GUARD = M.SENTINEL, 1024
SIZES = {"y": lambda R, N: R * 64, "stats": lambda R, N: R * 4, "crow": lambda R, N: R * 2, "dx": lambda R, N: R * 64,
         "dW": lambda R, N: N * 64}
ROW_WISE = ("y", "stats", "crow", "dx")


def _buffers(R, N):
    return {k: torch.full((n(R, N) + GUARD,), SENTINEL, device=DEV) for k, n in SIZES.items()}


def _untouched(t):
    return bool((t == t.new_tensor(SENTINEL)).all())


def _fwd(c, b, space, **over):
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    a = dict(x=c.x.data_ptr(), R=c.R, bank=c.bank.data_ptr(), n_items=c.n_items, lam=c.lam, y=b["y"].data_ptr(),
             stats=b["stats"].data_ptr(), ws=space.data_ptr(), ws_bytes=space.numel())
    a.update(over)
    return lib().hvpr_memory_train_fwd_f32(a["x"], a["R"], a["bank"], a["n_items"], a["lam"], a["y"], a["stats"], a["ws"], a["ws_bytes"],
                                           kernels._stream())


def _bwd(c, b, space, **over):
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    a = dict(x=c.x.data_ptr(), dy=c.dy.data_ptr(), R=c.R, bank=c.bank.data_ptr(), n_items=c.n_items, lam=c.lam,
             stats=b["stats"].data_ptr(), dx=b["dx"].data_ptr(), dW=b["dW"].data_ptr(), crow=b["crow"].data_ptr(), ws=space.data_ptr(),
             ws_bytes=space.numel())
    a.update(over)
    return lib().hvpr_memory_train_bwd_f32(a["x"], a["dy"], a["R"], a["bank"], a["n_items"], a["lam"], a["stats"], a["dx"], a["dW"],
                                           a["crow"], a["ws"], a["ws_bytes"], kernels._stream())


def _workspace(n_items, fill=0):
    from hvpr_amd._lib import lib
    need = lib().hvpr_memory_train_workspace_bytes(n_items)
    assert need == M.workspace_bytes(n_items)                # the packed bank and the 32 splits of the bound's dw_k
    return torch.full((need,), fill, dtype=torch.uint8, device=DEV)


def _run(c, fill=0):
    """Forward, then backward on what the forward returned, every output in a sentinel buffer (dW too: it is overwritten, not
    accumulated into) -> the outputs, the guards checked."""
    b, ws = _buffers(c.R, c.n_items), _workspace(c.n_items, fill)
    assert (_fwd(c, b, ws), _bwd(c, b, ws)) == (OK, OK)
    torch.cuda.synchronize()
    out = {}
    for k, n in SIZES.items():
        n = n(c.R, c.n_items)
        assert _untouched(b[k][n:]), (c.name, k, "wrote past its end")
        out[k] = b[k][:n].view(-1, {"y": 64, "stats": 4, "crow": 2, "dx": 64, "dW": 64}[k])
    return out


def _rows(c, idx):
    """The case with only the rows idx of x and dy, in that order."""
    d = c.to(DEV)
    d.x, d.dy, d.free, d.R = c.x[idx].contiguous(), c.dy[idx].contiguous(), c.free[idx], len(idx)
    return d


@pytest.mark.parametrize("name", list(M.ROWS))
def test_row_within_the_bound(name, observed):
    c = M.case(name).to(DEV)
    got, again, third = _run(c, 0), _run(c, 0xFF), _run(c, 0xFF)
    for k in got:
        assert torch.equal(got[k], again[k]) and torch.equal(again[k], third[k]), (name, k, "differs from call to call")
    r = M.reference(c)
    fr = M.fractions(got, r, c.free)
    observed(f"memory train [{name}] {c.R} x {c.n_items}: max err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in fr.items()))
    assert max(fr.values()) <= 1.0, (name, fr)
    assert bool((got["stats"][:, 3] == 0).all()), name
    for k in M.EXACT.get(name, ()):
        assert bool((got[k] == 0).all()), (name, k)
    if bool(c.free.any()):
        assert bool(torch.isfinite(got["y"][c.free]).all()) and bool(torch.isfinite(got["dx"][c.free]).all())
        assert bool((got["crow"][c.free] == 0).all())


@pytest.mark.parametrize("name", ["R65", "mixed_groups", "planted_borders", "near_threshold", "n17"])
def test_a_row_does_not_depend_on_its_neighbours(name):
    """The rows in reversed order, and the first 17 alone: another place in the group of 16, another workgroup (another rotation of
    the item tiles over the waves), other neighbours — the same bits."""
    c = M.case(name).to(DEV)
    full = _run(c)
    rev = torch.arange(c.R - 1, -1, -1, device=DEV)
    got = _run(_rows(c, rev))
    for k in ROW_WISE:
        assert torch.equal(got[k], full[k][rev]), (name, k, "reversed")
    head = torch.arange(min(17, c.R), device=DEV)
    got = _run(_rows(c, head))
    for k in ROW_WISE:
        assert torch.equal(got[k], full[k][head]), (name, k, "the first 17 rows alone")


@pytest.mark.parametrize("name", ["R65", "n129", "empty_all"])
def test_autograd_function_gives_the_bits_of_the_direct_calls(name):
    from hvpr_amd.map_to_bev import _MemoryTrain
    c = M.case(name).to(DEV)
    want = _run(c)
    x, w = c.x.clone().requires_grad_(True), c.bank.clone().requires_grad_(True)
    y = _MemoryTrain.apply(x, w, c.lam)
    dx, dw = torch.autograd.grad(y, (x, w), c.dy)
    assert torch.equal(y.detach(), want["y"]) and torch.equal(dx, want["dx"]) and torch.equal(dw, want["dW"])


NAN = float("nan")
# name -> (entry points it applies to, the arguments changed, the status)
REFUSALS = {
    "n_items_0": ("fb", dict(n_items=0), INVALID),
    "n_items_2049": ("fb", dict(n_items=2049), UNSUPPORTED),
    "lambda_0": ("fb", dict(lam=0.0), UNSUPPORTED),
    "lambda_negative": ("fb", dict(lam=-0.0025), UNSUPPORTED),
    "lambda_nan": ("fb", dict(lam=NAN), UNSUPPORTED),
    "R_negative": ("fb", dict(R=-1), INVALID),
    "short_workspace": ("fb", dict(short=1), WORKSPACE),
    "null_x": ("fb", dict(x=0), INVALID),
    "null_bank": ("fb", dict(bank=0), INVALID),
    "null_workspace": ("fb", dict(ws=0), INVALID),
    "null_y": ("f", dict(y=0), INVALID),
    "null_stats_out": ("f", dict(stats=0), INVALID),
    "null_dy": ("b", dict(dy=0), INVALID),
    "null_stats_in": ("b", dict(stats=0), INVALID),
    "null_dx": ("b", dict(dx=0), INVALID),
    "null_dbank": ("b", dict(dW=0), INVALID),
    "null_row_scratch": ("b", dict(crow=0), INVALID),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_memory_train_refuses(name):
    """The buffers are those of the accepted 17 x 2000 call; the backward is handed the row statistics of that call.  The entry point
    refuses, and every output keeps its sentinel."""
    which, over, status = REFUSALS[name]
    c = M.case("R17").to(DEV)
    ws = _workspace(c.n_items)
    good = _buffers(c.R, c.n_items)
    assert (_fwd(c, good, ws), _bwd(c, good, ws)) == (OK, OK) and not any(_untouched(v[:16]) for v in good.values())
    over = dict(over)
    if "short" in over:
        over = dict(ws_bytes=ws.numel() - over["short"])
    b = _buffers(c.R, c.n_items)
    if "f" in which:
        assert _fwd(c, b, ws, **over) == status
    if "b" in which:
        assert _bwd(c, b, ws, **{"stats": good["stats"].data_ptr(), **over}) == status
    torch.cuda.synchronize()
    for k, v in b.items():
        assert _untouched(v), (name, k)


def test_no_rows():
    """R = 0: the forward is OK and writes nothing; the backward writes dbank exactly 0 over its sentinel and leaves dx alone."""
    c = M.case("R17").to(DEV)
    ws = _workspace(c.n_items, 0xFF)
    b = _buffers(c.R, c.n_items)
    assert _fwd(c, b, ws, R=0) == OK
    torch.cuda.synchronize()
    assert all(_untouched(v) for v in b.values())
    assert _bwd(c, b, ws, R=0) == OK
    torch.cuda.synchronize()
    n = c.n_items * 64
    assert bool((b["dW"][:n] == 0).all()) and _untouched(b["dW"][n:])
    assert all(_untouched(b[k]) for k in ("y", "stats", "crow", "dx"))
