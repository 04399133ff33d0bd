"""Fixture G28 (tests/golden/g28_pointpillar.npz): plain PointPillars' eval forward on the reference's own modules.

Runs ONLY in the build container (needs /root/reference; CPU torch), like make_golden.py, whose in-memory loader it uses.
Parameters are detparams tensors by name and seed (tests/pointpillar_cases.load_det), so only names and shapes are stored.

  vfe.A / vfe.B   PillarVFE eval (pillar_vfe.py:94-124).  A: NUM_FILTERS [64], P = 32, M = 200 (make_golden.synth_voxels, n = 1 and
                  n = P forced); B: [128], P = 20, M = 64.  Inputs, pillar_features, pillar_mask.  Each case is asserted to hold
                  (pillar, channel) pairs whose maximum is the padded slot's relu(b[c]) and pairs whose maximum is a live slot's
                  (the quirk is pinned only with both); the two counts are stored (pad_wins, live_wins).
  bev.small / bev.full   BaseBEVBackbone eval (base_bev_backbone.py:81-113), batch 2, sparse non-negative input as in G4.
                  small: 32 -> [32, 48, 64], LAYER_NUMS [1, 2, 2], LAYER_STRIDES [1, 2, 2], 20 x 28, upsample filters [32, 32, 32];
                  full: 64 -> [64, 128, 256], [3, 5, 5], [2, 2, 2], 16 x 24, [128, 128, 128]; UPSAMPLE_STRIDES [1, 2, 4].
  chain           PillarVFE -> PointPillarScatter -> BaseBEVBackbone -> AnchorHeadSingle with pointpillar.yaml's model settings on a
                  24 x 16 grid (head 12 x 8, 576 anchors), M = 120 pillars, batch 2: the voxel inputs, batch_cls_preds, batch_box_preds.

Usage:  python tests/golden/make_golden_pointpillar.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import make_golden as G  # noqa: E402
from make_golden import EasyDict  # noqa: E402

import pointpillar_cases as PC  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g28_pointpillar.npz")
CHAIN_RANGE = [0, -19.84, -2.5, 3.84, -17.28, 0.5]          # synth_voxels' origin and voxel size: 24 x 16 cells of 0.16 m


def _names(shapes, prefix=""):
    return {"param_names": np.array([prefix + k for k in shapes]), "param_shapes": np.array([str(list(v)) for v in shapes.values()])}


def _det(module, seed, prefix=""):
    shapes = {prefix + k: tuple(v.shape) for k, v in module.state_dict().items() if "num_batches_tracked" not in k}
    PC.load_det(module, shapes, seed, prefix)
    return shapes


def _vfe_cfg(filters):
    return EasyDict(USE_NORM=True, WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, NUM_FILTERS=filters)


def vfe_cases(R, out):
    for tag, (filters, P, M, seed) in {"A": ([64], 32, 200, 2801), "B": ([128], 20, 64, 2802)}.items():
        gen = torch.Generator().manual_seed(seed)
        m = R.pillar_vfe.PillarVFE(model_cfg=_vfe_cfg(filters), num_point_features=4, voxel_size=G.VOXEL_SIZE, point_cloud_range=G.PC_RANGE)
        shapes = _det(m, seed)
        m.eval()
        vox, n, coords = G.synth_voxels(gen, M, P=P)
        with torch.no_grad():
            d = m({"voxels": vox.clone(), "voxel_num_points": n.clone(), "voxel_coords": coords.clone()})
        feats, mask = d["pillar_features"].numpy(), d["pillar_mask"].numpy()
        assert feats.shape == (M, filters[0]) and mask.shape == (M, P, 1)
        # which slot holds the maximum, from the float64 restatement on the folded layer
        lin, bn = m.pfn_layers[0].linear, m.pfn_layers[0].norm
        with torch.no_grad():
            s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
            w = (lin.weight.double() * s[:, None]).float().numpy()
            b = (bn.bias.double() - bn.running_mean.double() * s).float().numpy()
        r = PC.pfn64(vox.numpy(), n.numpy(), coords.numpy(), w, b, G.VOXEL_SIZE, PC.offsets_of(G.VOXEL_SIZE, G.PC_RANGE))
        np.testing.assert_allclose(r["out"], feats, rtol=1e-3, atol=1e-4)
        live = r["mask"][..., None] > 0
        best_live = np.where(live, r["y"], -np.inf).max(axis=1)                 # (M, C)
        pad = np.broadcast_to(np.maximum(b.astype(np.float64), 0.0), best_live.shape)
        has_pad = (n.numpy() < P)[:, None]
        pad_wins = int((has_pad & (pad > best_live)).sum())
        live_wins = int((has_pad & (best_live > pad)).sum())
        assert pad_wins >= 1 and live_wins >= 1, (tag, pad_wins, live_wins)
        p = f"vfe.{tag}."
        out.update({p + "voxels": vox.numpy(), p + "voxel_num_points": n.numpy().astype(np.int32),
                    p + "voxel_coords": coords.numpy().astype(np.int32), p + "pillar_features": feats, p + "pillar_mask": mask,
                    p + "num_filters": np.array(filters), p + "param_seed": np.array(seed), p + "pad_wins": np.array(pad_wins),
                    p + "live_wins": np.array(live_wins), **{p + k: v for k, v in _names(shapes).items()}})
        print(f"G28 vfe.{tag}: pad_wins {pad_wins}, live_wins {live_wins}")


BEV_CASES = {
    "small": dict(C=32, NUM_FILTERS=[32, 48, 64], LAYER_NUMS=[1, 2, 2], LAYER_STRIDES=[1, 2, 2], H=20, W=28,
                  NUM_UPSAMPLE_FILTERS=[32, 32, 32], seed=2811),
    "full": dict(C=64, NUM_FILTERS=[64, 128, 256], LAYER_NUMS=[3, 5, 5], LAYER_STRIDES=[2, 2, 2], H=16, W=24,
                 NUM_UPSAMPLE_FILTERS=[128, 128, 128], seed=2812),
}


def _bev_cfg(c):
    return EasyDict(LAYER_NUMS=c["LAYER_NUMS"], LAYER_STRIDES=c["LAYER_STRIDES"], NUM_FILTERS=c["NUM_FILTERS"],
                    UPSAMPLE_STRIDES=[1, 2, 4], NUM_UPSAMPLE_FILTERS=c["NUM_UPSAMPLE_FILTERS"])


def bev_cases(R, out):
    for tag, c in BEV_CASES.items():
        gen = torch.Generator().manual_seed(c["seed"])
        m = R.bev.BaseBEVBackbone(model_cfg=_bev_cfg(c), input_channels=c["C"])
        shapes = _det(m, c["seed"])
        m.eval()
        occ = (torch.rand(2, 1, c["H"], c["W"], generator=gen) < 0.35).float()      # sparse, non-negative: like the scatter output
        x = torch.relu(torch.randn(2, c["C"], c["H"], c["W"], generator=gen)) * occ
        with torch.no_grad():
            d = m({"spatial_features": x.clone()})
        p = f"bev.{tag}."
        out.update({p + "spatial_features": x.numpy(), p + "spatial_features_2d": d["spatial_features_2d"].numpy(),
                    p + "layer_nums": np.array(c["LAYER_NUMS"]), p + "layer_strides": np.array(c["LAYER_STRIDES"]),
                    p + "upsample_strides": np.array([1, 2, 4]), p + "num_upsample_filters": np.array(c["NUM_UPSAMPLE_FILTERS"]),
                    p + "param_seed": np.array(c["seed"]), **{p + k: v for k, v in _names(shapes).items()}})


def chain_case(R, out):
    from hvpr_amd import config
    seed, nx, ny, M, B = 2821, 24, 16, 120, 2
    gen = torch.Generator().manual_seed(seed)
    model = config.pointpillar_cfg().MODEL
    rng = np.array(CHAIN_RANGE, dtype=np.float32)
    grid = np.array([nx, ny, 1])
    vfe = R.pillar_vfe.PillarVFE(model_cfg=_vfe_cfg(list(model.VFE.NUM_FILTERS)), num_point_features=4, voxel_size=G.VOXEL_SIZE,
                                 point_cloud_range=CHAIN_RANGE)
    scatter = R.scatter.PointPillarScatter(model_cfg=EasyDict(NUM_BEV_FEATURES=64), grid_size=grid)
    bev = R.bev.BaseBEVBackbone(model_cfg=EasyDict({k: v for k, v in model.BACKBONE_2D.items() if k != "NAME"}), input_channels=64)
    head = R.head_single.AnchorHeadSingle(model_cfg=EasyDict(dict(model.DENSE_HEAD)), input_channels=bev.num_bev_features, num_class=3,
                                          class_names=["Car", "Pedestrian", "Cyclist"], grid_size=grid, point_cloud_range=rng)
    shapes = {}
    for module, prefix in ((vfe, "vfe."), (bev, "backbone_2d."), (head, "dense_head.")):
        shapes.update(_det(module, seed, prefix))
        module.eval()
    vox, n, coords = G.synth_voxels(gen, M, P=32, nx=nx, ny=ny, batch=B)
    assert set(coords[:, 0].long().tolist()) == {0, 1}
    with torch.no_grad():
        d = {"voxels": vox.clone(), "voxel_num_points": n.clone(), "voxel_coords": coords.clone(), "batch_size": B}
        for module in (vfe, scatter, bev, head):
            d = module(d)
    cls, box = d["batch_cls_preds"].numpy(), d["batch_box_preds"].numpy()
    assert cls.shape == (B, 576, 3) and box.shape == (B, 576, 7), (cls.shape, box.shape)
    out.update({"chain.voxels": vox.numpy(), "chain.voxel_num_points": n.numpy().astype(np.int32),
                "chain.voxel_coords": coords.numpy().astype(np.int32), "chain.batch_cls_preds": cls, "chain.batch_box_preds": box,
                "chain.point_cloud_range": rng, "chain.voxel_size": np.array(G.VOXEL_SIZE, np.float32), "chain.grid": np.array([nx, ny]),
                "chain.param_seed": np.array(seed), **{"chain." + k: v for k, v in _names(shapes).items()}})


def main():
    R = G.load_reference()
    out = {}
    vfe_cases(R, out)
    bev_cases(R, out)
    chain_case(R, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
