"""Per-item work outside the K loops of the two forward convolution kernels (csrc/conv_wino.hip `k_wino<1, false, 2>`,
csrc/conv_igemm.hip `k_conv`): the walk's items come from a table built once per shape, the accumulators are born in the peeled first
chunk.  Nothing of this may change a bit of any output:

* the Winograd px_groups 1 launch with a table equals the same launch with a null table AND the px_groups 2 launch, a kernel
  instantiation the change does not touch (same fma chains: tests/test_gpu_wino_edge_pairs.py);
* the direct kernel with a table equals the same launch with a null table;
* the device tables equal a numpy restatement of csrc/wino_walk.h (and of the direct kernel's decode), entry for entry;
* a captured graph of a layer whose table was built eagerly replays to the eager result, and a capture that finds no table runs the
  null path without allocating."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 8 x 16: one plain item, seven holes in its round.  12 x 20: right and bottom pairs plus the corner.  9 x 40, two images: a ragged
# right column and a one-pixel bottom row, two images (pairs must not cross from one into the next).  17 x 33: odd pair counts leave
# a tile single.  All but 9 x 40 leave holes in the last round of the walk (their items are no multiple of 8).
IMAGES = [(1, 8, 16), (1, 12, 20), (2, 9, 40), (1, 17, 33)]
CINS = [8, 16, 24]            # one chunk (the peeled chunk is also the last) | the two-chunk body | the odd tail
COUTS = [4, 64, 68]           # a padded channel tile | a whole one | a second, ragged one


def _wino_case(N, H, W, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, cin, generator=g).to(DEV)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).to(DEV)
    scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    gate = torch.rand(N, H, W, generator=g).to(DEV)
    resid = torch.randn(N, H, W, cout, generator=g).to(DEV)
    return x, w, scale, shift, gate, resid


@pytest.mark.parametrize("N,H,W", IMAGES)
def test_winograd_with_table_equals_null_table_and_the_untouched_variant(N, H, W):
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    for cin in CINS:
        for cout in COUTS:
            x, w, scale, shift, gate, resid = _wino_case(N, H, W, cin, cout, H * 131 + W * 7 + cin + cout)
            gated = (cin + cout) % 3 != 0                  # gate + residual on two of three combinations, plain ReLU on the rest
            kw = dict(gate=gate, resid=resid) if gated else {}
            pc1 = kernels.pack_conv_wino(w, scale, shift, relu=True, px_groups=1)
            pc2 = kernels.pack_conv_wino(w, scale, shift, relu=True, px_groups=2)
            tag = f"{N}x{H}x{W} cin {cin} cout {cout} gated {gated}"
            y_tab = kernels.conv2d_wino_nhwc(x, pc1, use_table=True, **kw)
            assert (N, H, W) in pc1.tabs and pc1.tabs[(N, H, W)].numel() > 0, tag          # the table path did run
            items = lib().hvpr_conv2d_wino_items(N, H, W, cout, 1)
            assert pc1.tabs[(N, H, W)].numel() >= items, tag
            if (H, W) == (8, 16):
                assert pc1.tabs[(N, H, W)].numel() == 8 * items, tag             # one item and seven holes per channel tile
            y_null = kernels.conv2d_wino_nhwc(x, pc1, use_table=False, **kw)
            y_g2 = kernels.conv2d_wino_nhwc(x, pc2, **kw)
            for name, y in (("null table", y_null), ("px_groups 2", y_g2)):
                diff = (y_tab - y).abs()
                print(f"{tag}: max |table - {name}| = {float(diff.max()):.3e}")
                assert torch.equal(y_tab, y), (tag, name, [tuple(i) for i in diff.amax(-1).nonzero()[:8].tolist()])
            # into a channel slice of a wider buffer: the same bits, the columns outside untouched
            wide = torch.full((N, H, W, cout + 24), 7.0, device=DEV)
            kernels.conv2d_wino_nhwc(x, pc1, out=wide, out_coff=12, use_table=True, **kw)
            assert torch.equal(wide[..., 12:12 + cout], y_tab), tag
            assert bool((wide[..., :12] == 7).all()) and bool((wide[..., 12 + cout:] == 7).all()), tag


def _direct_pair(x, pc, **kw):
    from hvpr_amd import kernels
    y_tab = kernels.conv2d_nhwc(x, pc, use_table=True, **kw)
    assert tuple(x.shape[:3]) in pc.tabs and pc.tabs[tuple(x.shape[:3])].numel() > 0
    y_null = kernels.conv2d_nhwc(x, pc, use_table=False, **kw)
    return y_tab, y_null


@pytest.mark.parametrize("tile_cfg", [0, 1, 2])
@pytest.mark.parametrize("cin", [8, 16])
def test_direct_stride2_with_table_equals_null_table(cin, tile_cfg):
    from hvpr_amd import kernels
    g = torch.Generator().manual_seed(cin + tile_cfg)
    x = torch.randn(2, 9, 11, cin, generator=g).to(DEV)                      # two images, 5 x 6 outputs
    w = (torch.randn(68, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).to(DEV)
    pc = kernels.pack_conv(w, (torch.rand(68, generator=g) + 0.5).to(DEV), (torch.randn(68, generator=g) * 0.1).to(DEV), stride=2,
                           relu=True, tile_cfg=tile_cfg)
    y_tab, y_null = _direct_pair(x, pc)
    assert y_tab.shape == (2, 5, 6, 68) and torch.equal(y_tab, y_null)


@pytest.mark.parametrize("tile_cfg", [0, 1, 2])
@pytest.mark.parametrize("cin", [32, 8])                                      # four chunks per stage | one
def test_direct_1x1_with_table_equals_null_table(cin, tile_cfg):
    from hvpr_amd import kernels
    g = torch.Generator().manual_seed(100 + cin + tile_cfg)
    x = torch.randn(2, 9, 19, cin, generator=g).to(DEV)
    w = (torch.randn(20, cin, 1, 1, generator=g) / np.sqrt(cin)).to(DEV)
    pc = kernels.pack_conv(w, None, (torch.randn(20, generator=g) * 0.1).to(DEV), relu=False, tile_cfg=tile_cfg)
    gate = torch.rand(2, 9, 19, generator=g).to(DEV)
    resid = torch.randn(2, 9, 19, 20, generator=g).to(DEV)
    y_tab, y_null = _direct_pair(x, pc, gate=gate, resid=resid)
    assert torch.equal(y_tab, y_null)


@pytest.mark.parametrize("cin", [32, 8])
def test_direct_deconv_into_a_channel_slice_with_table_equals_null_table(cin):
    from hvpr_amd import kernels
    g = torch.Generator().manual_seed(200 + cin)
    x = torch.randn(2, 9, 11, cin, generator=g).to(DEV)
    w = (torch.randn(cin, 12, 2, 2, generator=g) / np.sqrt(cin)).to(DEV)
    pc = kernels.pack_deconv(w, (torch.rand(12, generator=g) + 0.5).to(DEV), (torch.randn(12, generator=g) * 0.1).to(DEV), relu=True, tile_cfg=1)
    wide_tab = torch.full((2, 18, 22, 36), 7.0, device=DEV)
    wide_null = wide_tab.clone()
    kernels.conv2d_nhwc(x, pc, out=wide_tab, out_coff=8, use_table=True)
    assert pc.tabs[(2, 9, 11)].numel() > 0
    kernels.conv2d_nhwc(x, pc, out=wide_null, out_coff=8, use_table=False)
    assert torch.equal(wide_tab, wide_null)
    assert bool((wide_tab[..., :8] == 7).all()) and bool((wide_tab[..., 20:] == 7).all()) and not bool((wide_tab[..., 8:20] == 7).any())


# ---- the tables, entry for entry -------------------------------------------------------------------------------------------------
def _walk_make(H, W):
    """csrc/wino_walk.h, wino_walk_make(H, W, 8, pairing = 1)"""
    tiles_x, tiles_y = (W + 15) // 16, (H + 7) // 8
    live_bcols = (W - 16 * (tiles_x - 1) + 1) // 2
    live_brows = (H - 8 * (tiles_y - 1) + 1) // 2
    rp, bp = live_bcols <= 4, live_brows <= 2
    wi, hi = (tiles_x - 1 if rp else tiles_x), (tiles_y - 1 if bp else tiles_y)
    n_plain, n_right = wi * hi, ((tiles_y + 1) // 2 if rp else 0)
    return dict(tiles_x=tiles_x, tiles_y=tiles_y, wi=wi, hi=hi, n_plain=n_plain, n_right=n_right,
                per_image=n_plain + n_right + ((wi + 1) // 2 if bp else 0))


def _walk_table_numpy(N, H, W, cout):
    """conv_walk_step + wino_walk_item + the packing of wino_tab_entry, per step"""
    w = _walk_make(H, W)
    n_ct = (cout + 63) // 64
    n_pt = N * w["per_image"]
    steps = (n_pt + 7) // 8 * 8 * n_ct
    out = np.zeros(steps, np.uint64)
    for it in range(steps):
        xcd, j = it & 7, it >> 3
        ct, pt = j % n_ct, (j // n_ct) * 8 + xcd
        if pt >= n_pt:
            out[it] = 1 << 31
            continue
        n, q = pt // w["per_image"], pt % w["per_image"]
        if q < w["n_plain"]:
            ty, tx, mode = q // w["wi"], q % w["wi"], 0
        elif q - w["n_plain"] < w["n_right"]:
            ty, tx = 2 * (q - w["n_plain"]), w["tiles_x"] - 1
            mode = 1 if ty + 1 < w["tiles_y"] else 0
        else:
            ty, tx = w["tiles_y"] - 1, 2 * (q - w["n_plain"] - w["n_right"])
            mode = 2 if tx + 1 < w["wi"] else 0
        out[it] = (tx | ty << 12 | mode << 24) | (ct | n << 12) << 32
    return out, n_ct


@pytest.mark.parametrize("N,H,W,cout", [(N, H, W, c) for (N, H, W) in IMAGES for c in COUTS]
                         + [(1, 248, 296, 128), (1, 124, 148, 256), (1, 62, 74, 512)])
def test_winograd_table_equals_the_walk_restated_in_numpy(N, H, W, cout):
    from hvpr_amd import kernels
    from hvpr_amd._lib import check, lib
    L = lib()
    want, n_ct = _walk_table_numpy(N, H, W, cout)
    items = L.hvpr_conv2d_wino_items(N, H, W, cout, 1)
    assert items % n_ct == 0 and len(want) == (items // n_ct + 7) // 8 * 8 * n_ct      # the walk's rounding: whole rounds of 8 pixel items
    assert L.hvpr_conv2d_wino_tab_bytes(N, H, W, cout, 1) == 8 * len(want)
    assert int((want >> np.uint64(31) & np.uint64(1)).sum()) == len(want) - items       # every step is an item or a hole
    t = torch.full((len(want) + 1,), -1, dtype=torch.int64, device=DEV)
    check(L.hvpr_conv2d_wino_tab_build(N, H, W, cout, 1, t.data_ptr(), kernels._stream()), "hvpr_conv2d_wino_tab_build")
    got = t.cpu().numpy()
    assert got[-1] == -1                                                                # nothing behind the table is written
    assert np.array_equal(got[:-1].view(np.uint64), want)
    for groups in (2, 4):                                                               # no table for the untouched variants
        assert L.hvpr_conv2d_wino_tab_bytes(N, H, W, cout, groups) == 0


@pytest.mark.parametrize("N,H,W,taps,stride,cout_pad,tile_cfg", [(2, 9, 11, 9, 2, 128, 0), (2, 9, 11, 9, 2, 128, 1), (2, 9, 19, 1, 1, 64, 2),
                                                                 (1, 248, 296, 9, 2, 256, 1), (1, 62, 74, 1, 1, 512, 1)])
def test_direct_table_equals_the_decode_restated_in_numpy(N, H, W, taps, stride, cout_pad, tile_cfg):
    from hvpr_amd import kernels
    from hvpr_amd._lib import check, lib
    L = lib()
    OH, OW = ((H - 1) // stride + 1, (W - 1) // stride + 1) if taps == 9 else (H, W)
    tw, bn = (8 if tile_cfg == 1 else 16), (128 if tile_cfg == 0 else 64)
    tiles_x, tiles_y, n_ct = (OW + tw - 1) // tw, (OH + 7) // 8, cout_pad // bn
    n_pt = N * tiles_x * tiles_y
    it = np.arange((n_pt + 7) // 8 * 8 * n_ct, dtype=np.int64)
    ct, pt = (it >> 3) % n_ct, ((it >> 3) // n_ct) * 8 + (it & 7)
    tx, ty, n = pt % tiles_x, pt // tiles_x % tiles_y, pt // tiles_x // tiles_y
    want = np.where(pt >= n_pt, 1 << 31, (tx | ty << 16) | (ct | n << 12) << 32)
    assert L.hvpr_conv2d_tab_bytes(N, H, W, taps, stride, cout_pad, tile_cfg) == 8 * len(want)
    t = torch.full((len(want) + 1,), -1, dtype=torch.int64, device=DEV)
    check(L.hvpr_conv2d_tab_build(N, H, W, taps, stride, cout_pad, tile_cfg, t.data_ptr(), kernels._stream()), "hvpr_conv2d_tab_build")
    got = t.cpu().numpy()
    assert got[-1] == -1 and np.array_equal(got[:-1], want)


# ---- graph capture ---------------------------------------------------------------------------------------------------------------
def _capture(fn):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        fn()
    return graph


def test_capture_replays_the_eagerly_built_table_and_never_builds_one():
    from hvpr_amd import kernels
    N, H, W, cin, cout = 1, 12, 20, 16, 68
    x, w, scale, shift, gate, resid = _wino_case(N, H, W, cin, cout, 77)
    out = torch.empty(N, H, W, cout, device=DEV)

    # table built by an eager call first: the capture bakes its address in and replays to the eager result
    pc = kernels.pack_conv_wino(w, scale, shift, relu=True, px_groups=1)
    eager = kernels.conv2d_wino_nhwc(x, pc, gate=gate, resid=resid, use_table=True).clone()
    table = pc.tabs[(N, H, W)]
    torch.cuda.synchronize()
    graph = _capture(lambda: kernels.conv2d_wino_nhwc(x, pc, out=out, gate=gate, resid=resid, use_table=True))
    assert pc.tabs[(N, H, W)] is table
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)

    # no table cached: the call inside the capture takes the null path, builds and allocates nothing
    pc_cold = kernels.pack_conv_wino(w, scale, shift, relu=True, px_groups=1)
    kernels.conv2d_wino_nhwc(x, pc_cold, out=out, gate=gate, resid=resid, use_table=False)        # lazy kernel set-up outside the capture
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    graph_cold = _capture(lambda: kernels.conv2d_wino_nhwc(x, pc_cold, out=out, gate=gate, resid=resid, use_table=True))
    assert pc_cold.tabs == {} and torch.cuda.memory_allocated() == before
    out.fill_(float("nan"))
    graph_cold.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
