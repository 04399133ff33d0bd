"""Paired ragged edge tiles of hvpr_conv2d_wino_nhwc_f32 (csrc/wino_walk.h): two right-edge tiles with <= 4 live block columns, or two
bottom-edge tiles with <= 2 live block rows, are computed by one workgroup item.

EMBEDDING ORACLE, bit for bit: the output on a ragged image equals the crop of the same kernel's output on that image embedded
top-left in a zero canvas whose height is a multiple of 8 and width a multiple of 16 — full tiles only, so nothing is paired there.
Every output element is the same k-ordered fma chain both ways and the halo beyond the image is zero both ways, so the comparison
is exact.  The same outputs are also held against a float64 direct convolution at the tolerance of tests/test_gpu_conv_wino.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# right pairing: 1, 2, 3, 4 live block columns in the last tile column pair, 5 must not (W = 26), W = 40 pairs behind two full
# columns; H = 16 / 24: an even / odd number of tile rows (the odd one leaves a single tile in front of the next image's first pair)
RIGHT = [(H, W) for W in (18, 20, 22, 24, 26, 40) for H in (16, 24)]
# bottom pairing: 1, 2 live block rows in the last tile row pair, 3 must not (H = 14), H = 20 pairs below two full rows;
# W = 32 / 48: an even / odd number of bottom tiles (full width: no right pairing)
BOTTOM = [(H, W) for H in (10, 12, 14, 20) for W in (32, 48)]
CORNER = [(12, 20), (12, 36), (20, 52)]      # both modes at once: the corner tile goes to the right pairing
# (cin, cout, relu, gate + residual): every value of each parameter with every value of each other one; cout 32 is padded to a
# 64-channel tile, cout 128 is two channel tiles per item
CONFIGS = [(8, 64, False, False), (16, 32, True, True), (16, 64, True, False), (8, 32, False, True), (8, 128, True, True)]


def _float64(x, w, scale, shift, relu, gate, resid):
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double() * scale.double().view(-1, 1, 1, 1), padding=1).permute(0, 2, 3, 1)
    y = y + shift.double()
    if relu:
        y = torch.relu(y)
    if gate is not None:
        y = gate.double().unsqueeze(-1) * y + resid.double()
    return y


def _embed(t, Hc, Wc):
    if t is None:
        return None
    c = torch.zeros((t.shape[0], Hc, Wc) + tuple(t.shape[3:]), dtype=t.dtype, device=t.device)
    c[:, :t.shape[1], :t.shape[2]] = t
    return c


@pytest.mark.parametrize("H,W", RIGHT + BOTTOM + CORNER)
def test_paired_edge_tiles_equal_the_embedded_full_tile_canvas(H, W):
    from hvpr_amd import kernels
    N = 2                                                     # two different images: a pair must not cross from one into the next
    Hc, Wc = (H + 7) // 8 * 8, (W + 15) // 16 * 16
    for cin, cout, relu, gated in CONFIGS:
        g = torch.Generator().manual_seed(H * 131 + W * 7 + cin + cout)
        x = torch.randn(N, H, W, cin, generator=g).to(DEV)
        w = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).to(DEV)
        scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
        shift = (torch.randn(cout, generator=g) * 0.1).to(DEV)
        gate = torch.rand(N, H, W, generator=g).to(DEV) if gated else None
        resid = torch.randn(N, H, W, cout, generator=g).to(DEV) if gated else None
        pc = kernels.pack_conv_wino(w, scale, shift, relu=relu, px_groups=1)
        y = kernels.conv2d_wino_nhwc(x, pc, gate=gate, resid=resid)
        canvas = kernels.conv2d_wino_nhwc(_embed(x, Hc, Wc), pc, gate=_embed(gate, Hc, Wc), resid=_embed(resid, Hc, Wc))
        tag = f"{H}x{W} cin {cin} cout {cout} relu {relu} gated {gated}"
        diff = (y - canvas[:, :H, :W]).abs()
        print(f"{tag}: max |ragged - canvas crop| = {float(diff.max()):.3e}")
        assert torch.equal(y, canvas[:, :H, :W]), (tag, [tuple(i) for i in diff.amax(-1).nonzero()[:8].tolist()])
        ref = _float64(x, w, scale, shift, relu, gate, resid)
        err = float((y.double() - ref).abs().max()) / float(ref.abs().max())
        print(f"{tag}: max abs error / output scale against float64 = {err:.2e}")
        assert err < 5e-6, (tag, err)
        # into a channel slice of a wider buffer: the slice is the same bits, the columns outside it are untouched
        wide = torch.full((N, H, W, cout + 24), 7.0, device=DEV)
        kernels.conv2d_wino_nhwc(x, pc, out=wide, out_coff=12, gate=gate, resid=resid)
        assert torch.equal(wide[..., 12:12 + cout], y), tag
        assert bool((wide[..., :12] == 7).all()) and bool((wide[..., 12 + cout:] == 7).all()), tag


def _tiles(H, W, th=8):
    return ((H + th - 1) // th) * ((W + 15) // 16)


def test_item_count_of_the_three_backbone_levels():
    from hvpr_amd._lib import lib
    L = lib()
    # level 0: 31 x 19 tiles, right column (4 of 8 block columns live) in 15 pairs + 1; level 1: 16 x 10 tiles, 8 right pairs, 4
    # bottom pairs + 1; level 2 (5 live block columns, 3 live block rows) cannot pair
    assert L.hvpr_conv2d_wino_items(1, 248, 296, 128, 1) == 574 * 2
    assert L.hvpr_conv2d_wino_items(1, 124, 148, 256, 1) == 148 * 4
    assert L.hvpr_conv2d_wino_items(1, 62, 74, 512, 1) == 40 * 8
    assert L.hvpr_conv2d_wino_items(3, 124, 148, 256, 1) == 3 * 148 * 4          # pairs never span images: N times one image
    assert L.hvpr_conv2d_wino_items(1, 124, 148, 36, 1) == 148                   # cout padded to one 64-channel tile
    assert L.hvpr_conv2d_wino_items(0, 8, 16, 64, 1) == 0 and L.hvpr_conv2d_wino_items(1, 8, 16, 64, 3) == 0


@pytest.mark.parametrize("H,W,items", [
    (16, 24, 3),      # 2 x 2 tiles, 4 live block columns: the right column is one pair
    (16, 26, 4),      # 5 live block columns: must not pair
    (16, 19, 3),      # odd width: columns 16..18 are 1.5 blocks = 2 live block columns (the second half live): pairs
    (16, 25, 4),      # 4.5 blocks = 5 live block columns: must not pair
    (12, 32, 3),      # 2 live block rows: the bottom row is one pair
    (14, 32, 4),      # 3 live block rows: must not pair
    (13, 32, 4),      # 2.5 blocks = 3 live block rows: must not pair
    (12, 20, 3),      # both conditions, 2 x 2 tiles: 1 plain + the right pair (with the corner) + the bottom row's single tile
    (24, 18, 5),      # 3 x 2 tiles, 1 live block column: 3 plain + one right pair + the odd row's single tile
])
def test_item_count_pins_the_pairing_condition(H, W, items):
    from hvpr_amd._lib import lib
    assert lib().hvpr_conv2d_wino_items(1, H, W, 64, 1) == items
    assert lib().hvpr_conv2d_wino_items(2, H, W, 128, 1) == 2 * 2 * items


@pytest.mark.parametrize("N,H,W,cout", [(1, 248, 296, 128), (1, 124, 148, 256), (2, 62, 74, 512), (2, 12, 20, 68), (3, 24, 18, 64)])
def test_item_count_of_the_unpaired_variants_is_the_tile_count(N, H, W, cout):
    from hvpr_amd._lib import lib
    L = lib()
    cp = (cout + 63) // 64 * 64
    assert L.hvpr_conv2d_wino_items(N, H, W, cout, 2) == N * _tiles(H, W, 16) * (cp // 64)
    assert L.hvpr_conv2d_wino_items(N, H, W, cout, 4) == N * _tiles(H, W) * (cp // 32)
    assert L.hvpr_conv2d_wino_stats_rows(N, H, W) == N * _tiles(H, W)            # the statistics launch: one item per row and channel tile


@pytest.mark.parametrize("groups", [2, 4])
def test_unpaired_variants_on_a_shape_that_would_pair(groups):
    """px_groups 2 / 4 keep one item per tile: same bits as the paired px_groups 1 launch (same fma chains) on 12 x 20 x 2 images."""
    from hvpr_amd import kernels
    g = torch.Generator().manual_seed(groups)
    x = torch.randn(2, 12, 20, 16, generator=g).to(DEV)
    w = (torch.randn(64, 16, 3, 3, generator=g) / 12.0).to(DEV)
    y1 = kernels.conv2d_wino_nhwc(x, kernels.pack_conv_wino(w, relu=False, px_groups=1))
    yg = kernels.conv2d_wino_nhwc(x, kernels.pack_conv_wino(w, relu=False, px_groups=groups))
    assert torch.equal(y1, yg)


def test_fused_statistics_launch_on_a_shape_that_would_pair():
    """The statistics variant keeps its tile grid: hvpr_conv2d_wino_stats_rows rows, sums equal to those of the paired launch's output."""
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    g = torch.Generator().manual_seed(5)
    N, H, W, cin, cout = 2, 12, 20, 16, 64
    x = torch.randn(N, H, W, cin, generator=g).to(DEV)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / 12.0).to(DEV)
    pc = kernels.pack_conv_wino(w, relu=False, px_groups=1)
    rows = lib().hvpr_conv2d_wino_stats_rows(N, H, W)
    part = torch.full((rows, 2, cout), float("nan"), device=DEV)
    ys = kernels.conv2d_wino_nhwc(x, pc, bn_partials=part)
    y = kernels.conv2d_wino_nhwc(x, pc)
    assert torch.equal(ys, y)
    assert bool(torch.isfinite(part).all())
    # a tile's fp32 sum is a chain of at most 32 + 3 additions (and one rounding of the square): |error| <= 36 * 2^-24 * sum |v|
    s1, s2, a1 = y.double().sum((0, 1, 2)), (y.double() ** 2).sum((0, 1, 2)), y.double().abs().sum((0, 1, 2))
    assert bool(((part[:, 0].double().sum(0) - s1).abs() <= 36 * 2.0 ** -24 * a1).all())
    assert bool(((part[:, 1].double().sum(0) - s2).abs() <= 37 * 2.0 ** -24 * s2).all())
