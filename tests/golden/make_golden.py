"""Generate the golden fixtures under tests/golden/ by IMPORTING the reference's own Python modules.

Runs ONLY in the build container (needs /root/reference; CPU torch).  The reference never travels:
what is committed is data — seeded inputs and the reference's outputs — as small .npz files.

The reference snapshot is not importable as a package: leaf files are loaded
through stub packages, and the in-memory shims of SURVEY.md §8c are applied:
  * memory_module.py: line 75 (a stray comment fragment, SyntaxError) dropped and the signature
    `forward(self, input1, input2, k)` turned into `forward(self, input1, k, input2=None)` — the
    form its callers use (pointpillar_scatter.py:133,200);
  * base_bev_backbone.py: `SpatialAttention` injected (missing import at :220);
  * anchor code: `torch.Tensor.cuda` -> identity, stub modules for the absent pcdet.ops.*;
  * numpy aliases np.int / np.bool for the dead branches that still parse them.

Usage:  python tests/golden/make_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from detparams import det_state  # noqa: E402

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


class EasyDict(dict):
    """Minimal stand-in for easydict.EasyDict (absent here)."""

    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in dict(d or {}, **kw).items():
            self[k] = v

    def __setitem__(self, k, v):
        if isinstance(v, dict) and not isinstance(v, EasyDict):
            v = EasyDict(v)
        elif isinstance(v, (list, tuple)):
            v = [EasyDict(x) if isinstance(x, dict) else x for x in v]
        super().__setitem__(k, v)

    __setattr__ = __setitem__

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _import_oracle():
    """The build's CPU oracle (C routines for the rotated geometry the reference does not ship).  Found next to this script's
    tests/ directory, or — when the script was copied elsewhere — in $HVPR_REPO, the working directory or /root/repo."""
    for root in (os.path.dirname(os.path.dirname(OUT)), os.environ.get("HVPR_REPO", ""), os.getcwd(), "/root/repo"):
        if root and os.path.isdir(os.path.join(root, "oracle")):
            if root not in sys.path:
                sys.path.insert(0, root)
            break
    from oracle import hvpr_oracle as O
    return O


def _stub(name, path=None):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    sys.modules[name] = m
    return m


def _load(name, file, patch=None):
    path = os.path.join(REF, file)
    if patch is None:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    src = patch(open(path).read())
    mod = types.ModuleType(name)
    mod.__file__ = path
    mod.__package__ = name.rpartition(".")[0]
    sys.modules[name] = mod
    exec(compile(src, path, "exec"), mod.__dict__)
    return mod


def load_reference():
    if not hasattr(np, "int"):
        np.int = int
    if not hasattr(np, "bool"):
        np.bool = bool
    torch.Tensor.cuda = lambda self, *a, **k: self
    for pkg, p in [("pcdet", "pcdet"), ("pcdet.models", "pcdet/models"), ("pcdet.utils", "pcdet/utils"),
                   ("pcdet.ops", None), ("pcdet.ops.iou3d_nms", None), ("pcdet.ops.roiaware_pool3d", None),
                   ("pcdet.models.backbones_3d", "pcdet/models/backbones_3d"),
                   ("pcdet.models.backbones_3d.vfe", "pcdet/models/backbones_3d/vfe"),
                   ("pcdet.models.backbones_2d", "pcdet/models/backbones_2d"),
                   ("pcdet.models.backbones_2d.map_to_bev", "pcdet/models/backbones_2d/map_to_bev"),
                   ("pcdet.models.dense_heads", "pcdet/models/dense_heads"),
                   ("pcdet.models.dense_heads.target_assigner", "pcdet/models/dense_heads/target_assigner"),
                   ("torchvision", None), ("torchvision.ops", None), ("torchvision.ops.boxes", None)]:
        _stub(pkg, os.path.join(REF, p) if p else os.path.join(REF, "_absent"))
    sys.modules["pcdet.ops.iou3d_nms"].iou3d_nms_utils = _stub("pcdet.ops.iou3d_nms.iou3d_nms_utils")
    sys.modules["pcdet.ops.roiaware_pool3d"].roiaware_pool3d_utils = _stub("pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils")
    sys.modules["torchvision.ops.boxes"].box_area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    sys.modules["pcdet.ops"].iou3d_nms = sys.modules["pcdet.ops.iou3d_nms"]
    sys.modules["pcdet.ops"].roiaware_pool3d = sys.modules["pcdet.ops.roiaware_pool3d"]

    R = types.SimpleNamespace()
    R.vfe_template = _load("pcdet.models.backbones_3d.vfe.vfe_template", "pcdet/models/backbones_3d/vfe/vfe_template.py")
    R.pillar_vfe = _load("pcdet.models.backbones_3d.vfe.pillar_vfe", "pcdet/models/backbones_3d/vfe/pillar_vfe.py")

    def patch_mem(src):
        lines = src.split("\n")
        assert "Mem, (TxM) x (MxC) = TxC" in lines[74], lines[74]
        del lines[74]
        src = "\n".join(lines)
        assert "def forward(self, input1, input2, k):" in src
        return src.replace("def forward(self, input1, input2, k):", "def forward(self, input1, k, input2=None):")

    R.memory_module = _load("pcdet.models.backbones_2d.map_to_bev.memory_module",
                            "pcdet/models/backbones_2d/map_to_bev/memory_module.py", patch_mem)
    R.scatter = _load("pcdet.models.backbones_2d.map_to_bev.pointpillar_scatter",
                      "pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py")
    R.spatial_attention = _load("pcdet.models.backbones_2d.spatial_attention", "pcdet/models/backbones_2d/spatial_attention.py")
    R.bev = _load("pcdet.models.backbones_2d.base_bev_backbone", "pcdet/models/backbones_2d/base_bev_backbone.py")
    R.bev.SpatialAttention = R.spatial_attention.SpatialAttention
    R.common_utils = _load("pcdet.utils.common_utils", "pcdet/utils/common_utils.py")
    R.box_coder_utils = _load("pcdet.utils.box_coder_utils", "pcdet/utils/box_coder_utils.py")
    sys.modules["pcdet.utils"].common_utils = R.common_utils
    sys.modules["pcdet.utils"].box_coder_utils = R.box_coder_utils
    R.box_utils = _load("pcdet.utils.box_utils", "pcdet/utils/box_utils.py",
                        lambda s: s.replace("from scipy.spatial.qhull import", "from scipy.spatial import"))
    sys.modules["pcdet.utils"].box_utils = R.box_utils
    R.loss_utils = _load("pcdet.utils.loss_utils", "pcdet/utils/loss_utils.py")
    sys.modules["pcdet.utils"].loss_utils = R.loss_utils
    R.anchor_generator = _load("pcdet.models.dense_heads.target_assigner.anchor_generator",
                               "pcdet/models/dense_heads/target_assigner/anchor_generator.py")
    R.atss = _load("pcdet.models.dense_heads.target_assigner.atss_target_assigner",
                   "pcdet/models/dense_heads/target_assigner/atss_target_assigner.py")
    R.axis_assigner = _load("pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner",
                            "pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py")
    R.head_template = _load("pcdet.models.dense_heads.anchor_head_template", "pcdet/models/dense_heads/anchor_head_template.py")
    R.head_single = _load("pcdet.models.dense_heads.anchor_head_single", "pcdet/models/dense_heads/anchor_head_single.py")
    return R


def randomise_bn(module, gen):
    """Non-trivial BN affine + running stats so that folding is exercised."""
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.weight.data = torch.empty_like(m.weight).uniform_(0.5, 1.5, generator=gen)
            m.bias.data = torch.empty_like(m.bias).normal_(0, 0.3, generator=gen)
            m.running_mean.data = torch.empty_like(m.running_mean).normal_(0, 0.5, generator=gen)
            m.running_var.data = torch.empty_like(m.running_var).uniform_(0.5, 2.0, generator=gen)


def load_det(module, seed):
    """Overwrite every parameter/buffer with the name-keyed deterministic tensors of detparams.py."""
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items() if "num_batches_tracked" not in k}
    st = det_state(shapes, seed)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
    return shapes


def sd_np(module):
    return {k: v.detach().cpu().numpy().copy() for k, v in module.state_dict().items() if "num_batches_tracked" not in k}


VOXEL_SIZE = [0.16, 0.16, 3.0]
PC_RANGE = [0, -19.84, -2.5, 47.36, 19.84, 0.5]


def synth_voxels(gen, M, P=32, nx=296, ny=248, batch=2):
    """Random pillars with n in [1,P] (n=1 and n=P forced), points inside their cell, zero-padded."""
    n = torch.randint(1, P + 1, (M,), generator=gen)
    n[0], n[1] = 1, P
    cells = torch.randperm(nx * ny, generator=gen)[:M]
    cx, cy = cells % nx, cells // nx
    b = torch.sort(torch.randint(0, batch, (M,), generator=gen))[0]
    coords = torch.stack([b, torch.zeros(M, dtype=torch.long), cy, cx], dim=1).float()
    u = torch.rand(M, P, 4, generator=gen)
    vox = torch.zeros(M, P, 4)
    vox[..., 0] = PC_RANGE[0] + (cx.view(-1, 1) + u[..., 0]) * VOXEL_SIZE[0]
    vox[..., 1] = PC_RANGE[1] + (cy.view(-1, 1) + u[..., 1]) * VOXEL_SIZE[1]
    vox[..., 2] = PC_RANGE[2] + u[..., 2] * VOXEL_SIZE[2]
    vox[..., 3] = u[..., 3]
    slot = torch.arange(P).view(1, -1)
    vox = vox * (slot < n.view(-1, 1)).unsqueeze(-1).float()
    return vox, n.float(), coords


def g1_vfe(R):
    gen = torch.Generator().manual_seed(101)
    cfg = EasyDict(USE_NORM=True, WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, NUM_FILTERS=[32, 64], NUM_SCALE_FEATURES=[16, 32])
    torch.manual_seed(101)
    m = R.pillar_vfe.PillarVFE_Scale(model_cfg=cfg, num_point_features=4, voxel_size=VOXEL_SIZE, point_cloud_range=PC_RANGE)
    randomise_bn(m, gen)
    vox, n, coords = synth_voxels(gen, 200)
    out = {}
    m.eval()
    with torch.no_grad():
        d = m({"voxels": vox.clone(), "voxel_num_points": n.clone(), "voxel_coords": coords.clone()})
    out.update(eval_pillar_features=d["pillar_features"].numpy(), eval_pillar_scale_features=d["pillar_scale_features"].numpy(),
               eval_pillar_mask=d["pillar_mask"].numpy())
    params_before = sd_np(m)
    m.train()
    with torch.no_grad():
        d = m({"voxels": vox.clone(), "voxel_num_points": n.clone(), "voxel_coords": coords.clone()})
    out.update(train_pillar_features=d["pillar_features"].numpy(), train_pillar_scale_features=d["pillar_scale_features"].numpy())
    after = sd_np(m)
    for k in after:
        if "running_" in k:
            out["after_train." + k] = after[k]
    np.savez_compressed(os.path.join(OUT, "g1_vfe.npz"), voxels=vox.numpy(), voxel_num_points=n.numpy(), voxel_coords=coords.numpy(),
                        **{"param." + k: v for k, v in params_before.items()}, **out)


def g2_g3_memory_scatter(R):
    gen = torch.Generator().manual_seed(202)
    nx, ny = 12, 10
    cfg = EasyDict(NUM_BEV_FEATURES=128, NUM_COORD_POINTS=3, NUM_PT_FEATURES=64, NUM_SCALE_FEATURES=32, NUM_K=20, NUM_M=2000,
                   SHRINK_TH=0.0025)
    torch.manual_seed(202)
    m = R.scatter.PointPillarScatter_Agg_Memory_1_scale(model_cfg=cfg, grid_size=np.array([nx, ny, 1]))
    load_det(m, 202)
    m.eval()
    M, B = 90, 2
    cells = torch.cat([torch.randperm(nx * ny, generator=gen)[:M // 2] for _ in range(B)])
    b = torch.arange(B).repeat_interleave(M // 2)
    coords = torch.stack([b, torch.zeros(M, dtype=torch.long), cells // nx, cells % nx], dim=1).float()
    pf = torch.relu(torch.randn(M, 64, generator=gen))          # post-ReLU pillar features are >= 0
    sf = torch.relu(torch.randn(M, 32, generator=gen))
    mask = torch.ones(M, 32, 1)
    with torch.no_grad():
        mem = m.memory(pf, 20)
        d = m({"pillar_features": pf.clone(), "pillar_scale_features": sf.clone(), "pillar_mask": mask, "voxel_coords": coords.clone()})
        logits = torch.nn.functional.linear(pf, m.memory.weight)
        topk = torch.topk(torch.softmax(logits, 1), 20, dim=1)[1]
    np.savez_compressed(os.path.join(OUT, "g2_memory_eval.npz"), f=pf.numpy(), W_seed=202, W_name="memory.weight", k=20,
                        output=mem["output"].numpy(), topk_idx=topk.numpy(),
                        logits_gap=(torch.sort(logits, 1, descending=True)[0][:, 19] - torch.sort(logits, 1, descending=True)[0][:, 20]).numpy())
    np.savez_compressed(os.path.join(OUT, "g3_scatter_eval.npz"), pillar_features=pf.numpy(), pillar_scale_features=sf.numpy(),
                        voxel_coords=coords.numpy(), W_seed=202, W_name="memory.weight", nx=nx, ny=ny, batch_size=B,
                        spatial_features=d["spatial_features"].numpy(), spatial_scale_features=d["spatial_scale_features"].numpy())


def g4_backbone(R):
    for tag, (C, filt, sfilt, H, W, seed) in {
        "small": (32, [32, 48, 64], [8, 16, 24], 16, 24, 404),     # channel counts the kernels take: multiples of 8
        "full": (128, [128, 256, 512], [32, 64, 128], 8, 12, 405),
    }.items():
        gen = torch.Generator().manual_seed(seed)
        cfg = EasyDict(LAYER_NUMS=[3, 3, 3], SFM_LAYER_NUMS=[3, 3, 3], LAYER_STRIDES=[1, 2, 2], NUM_FILTERS=filt,
                       NUM_SCALE_FILTERS=sfilt, UPSAMPLE_STRIDES=[1, 2, 4], NUM_UPSAMPLE_FILTERS=[filt[0]] * 3)
        torch.manual_seed(seed)
        m = R.bev.BaseBEVBackbone_Scale(model_cfg=cfg, input_channels=C)
        shapes = load_det(m, seed)
        m.eval()
        # sparse, non-negative canvases like the scatter output
        occ = (torch.rand(2, 1, H, W, generator=gen) < 0.35).float()
        x = torch.relu(torch.randn(2, C, H, W, generator=gen)) * occ
        y = torch.relu(torch.randn(2, C // 4, H, W, generator=gen)) * occ
        with torch.no_grad():
            d = m({"spatial_features": x.clone(), "spatial_scale_features": y.clone()})
        np.savez_compressed(os.path.join(OUT, f"g4_backbone_{tag}.npz"), spatial_features=x.numpy(), spatial_scale_features=y.numpy(),
                            layer_nums=[3, 3, 3], sfm_layer_nums=[3, 3, 3], layer_strides=[1, 2, 2], upsample_strides=[1, 2, 4],
                            spatial_features_2d=d["spatial_features_2d"].numpy(), param_seed=seed,
                            param_names=np.array(list(shapes.keys())), param_shapes=np.array([str(list(v)) for v in shapes.values()]))


GRAD_SAMPLE_STRIDE = 101        # "full" G4-train case: parameter gradients are kept as (norm, every 101st element)


def g4_backbone_train(R):
    """G4-train: base_bev_backbone.py:228-279 in TRAINING mode — both streams through the shared weights, batch
    statistics, every BatchNorm call updating its running statistics — on the reference's own module, CPU.  Stored: the fp32
    forward outputs and running statistics, and the gradients of the fixed scalar
        L = sum(spatial_features_2d * cot_f) + sum(spatial_features_point_2d * cot_fp)
    w.r.t. the three inputs and every parameter.  The gradients come from the SAME module in float64 (`.double()`, the
    yardstick: backward through 25 ReLU + train-BatchNorm layers is ill-conditioned in fp32) together with the norm-wise
    distance of the reference's own fp32 gradients from them (`ref32_err.*`), which documents the regime a fp32 implementation
    can be held to."""
    import copy
    for tag, (C, filt, sfilt, H, W, seed) in {
        "small": (32, [32, 48, 64], [8, 16, 24], 16, 24, 414),     # channel counts the kernels take: Cin % 8 == 0
        "full": (128, [128, 256, 512], [32, 64, 128], 8, 12, 415),
    }.items():
        gen = torch.Generator().manual_seed(seed)
        cfg = EasyDict(LAYER_NUMS=[3, 3, 3], SFM_LAYER_NUMS=[3, 3, 3], LAYER_STRIDES=[1, 2, 2], NUM_FILTERS=filt,
                       NUM_SCALE_FILTERS=sfilt, UPSAMPLE_STRIDES=[1, 2, 4], NUM_UPSAMPLE_FILTERS=[filt[0]] * 3)
        torch.manual_seed(seed)
        m = R.bev.BaseBEVBackbone_Scale(model_cfg=cfg, input_channels=C)
        shapes = load_det(m, seed)
        m.train()
        B = 2
        occ = (torch.rand(B, 1, H, W, generator=gen) < 0.35).float()
        occ_p = (torch.rand(B, 1, H, W, generator=gen) < 0.5).float()
        x = torch.relu(torch.randn(B, C, H, W, generator=gen)) * occ
        xp = torch.relu(torch.randn(B, C, H, W, generator=gen)) * occ_p
        y = torch.relu(torch.randn(B, C // 4, H, W, generator=gen)) * occ
        nf = 3 * filt[0]
        cot_f = torch.from_numpy(det_state({"cotangent.f": (B, nf, H, W)}, seed)["cotangent.f"])
        cot_fp = torch.from_numpy(det_state({"cotangent.fp": (B, nf, H, W)}, seed)["cotangent.fp"])
        res = {}
        for dt in (torch.float32, torch.float64):
            mm = copy.deepcopy(m).to(dt)
            ins = [t.clone().to(dt).requires_grad_(True) for t in (x, xp, y)]
            d = mm({"spatial_features": ins[0], "spatial_features_point": ins[1], "spatial_scale_features": ins[2]})
            f, fp = d["spatial_features_2d"], d["spatial_features_point_2d"]
            ((f * cot_f.to(dt)).sum() + (fp * cot_fp.to(dt)).sum()).backward()
            res[dt] = dict(f=f.detach(), fp=fp.detach(), gin=[t.grad for t in ins],
                           gpar={k: p.grad for k, p in mm.named_parameters()},
                           buf={k: v.detach().clone() for k, v in mm.named_buffers() if "num_batches" not in k},
                           nbt={k: int(v) for k, v in mm.named_buffers() if "num_batches" in k})
        r32, r64 = res[torch.float32], res[torch.float64]
        out = dict(spatial_features=x.numpy(), spatial_features_point=xp.numpy(), spatial_scale_features=y.numpy(),
                   layer_nums=[3, 3, 3], sfm_layer_nums=[3, 3, 3], layer_strides=[1, 2, 2], upsample_strides=[1, 2, 4],
                   param_seed=seed, param_names=np.array(list(shapes.keys())),
                   param_shapes=np.array([str(list(v)) for v in shapes.values()]),
                   spatial_features_2d=r32["f"].numpy(), spatial_features_point_2d=r32["fp"].numpy(),
                   spatial_features_2d_f64=r64["f"].float().numpy(), spatial_features_point_2d_f64=r64["fp"].float().numpy(),
                   grad_sample_stride=GRAD_SAMPLE_STRIDE if tag == "full" else 1)
        for k, v in r32["buf"].items():
            out["after_train." + k] = v.numpy()
        for k, v in r32["nbt"].items():
            out["num_batches_tracked." + k] = v

        def nerr(a, b):
            return float((a.double() - b).norm() / b.norm().clamp_min(1e-300))
        for name, g32, g64 in zip(("spatial_features", "spatial_features_point", "spatial_scale_features"), r32["gin"], r64["gin"]):
            out["grad_in." + name] = g64.float().numpy()
            out["ref32_err.grad_in." + name] = nerr(g32, g64)
        for k, g64 in r64["gpar"].items():
            g32 = r32["gpar"][k]
            out["grad_norm." + k] = float(g64.norm())
            # a conv bias in front of a train-mode BatchNorm has an exactly-zero gradient: only round-off on both sides
            out["ref32_err.grad." + k] = nerr(g32, g64) if float(g64.norm()) > 1e-9 * g64.numel() ** 0.5 else 0.0
            flat = g64.float().reshape(-1).numpy()
            out["grad." + k] = flat[::GRAD_SAMPLE_STRIDE].copy() if tag == "full" else g64.float().numpy()
        np.savez_compressed(os.path.join(OUT, f"g4_backbone_train_{tag}.npz"), **out)


def g5_head(R):
    gen = torch.Generator().manual_seed(505)
    for stride in (1, 2):
        nx, ny = 24, 16
        rng = np.array([0, -1.28, -2.5, 3.84, 1.28, 0.5], dtype=np.float32)
        head_cfg = EasyDict(
            CLASS_AGNOSTIC=False, USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
            ANCHOR_GENERATOR_CONFIG=[dict(class_name="Car", anchor_sizes=[[3.9, 1.6, 1.56]], anchor_rotations=[0, 1.57],
                                          anchor_bottom_heights=[-1.78], align_center=False, feature_map_stride=stride,
                                          matched_threshold=0.6, unmatched_threshold=0.45)],
            TARGET_ASSIGNER_CONFIG=dict(NAME="AxisAlignedTargetAssigner", POS_FRACTION=-1.0, SAMPLE_SIZE=512,
                                        NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False, BOX_CODER="ResidualCoder"),
            LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, mem_weight=1.0,
                                               code_weights=[1.0] * 7)))
        torch.manual_seed(505)
        m = R.head_single.AnchorHeadSingle(model_cfg=head_cfg, input_channels=48, num_class=1, class_names=["Car"],
                                           grid_size=np.array([nx, ny, 1]), point_cloud_range=rng)
        m.conv_box.weight.data.normal_(0, 0.05, generator=gen)
        m.conv_dir_cls.weight.data.normal_(0, 0.2, generator=gen)
        m.eval()
        H, W = ny // stride, nx // stride
        x = torch.randn(2, 48, H, W, generator=gen)
        with torch.no_grad():
            d = m({"spatial_features_2d": x.clone(), "batch_size": 2})
        np.savez_compressed(os.path.join(OUT, f"g5_head_stride{stride}.npz"), spatial_features_2d=x.numpy(), nx=nx, ny=ny,
                            stride=stride, point_cloud_range=rng, anchors=m.anchors[0].numpy(),
                            cls_preds=m.forward_ret_dict["cls_preds"].numpy(), box_preds=m.forward_ret_dict["box_preds"].numpy(),
                            dir_cls_preds=m.forward_ret_dict["dir_cls_preds"].numpy(),
                            batch_cls_preds=d["batch_cls_preds"].numpy(), batch_box_preds=d["batch_box_preds"].numpy(),
                            **{"param." + k: v for k, v in sd_np(m).items()})
    # full-size anchor grid of hvpr_car (stride 1): keep only a checksum + a strided sample (the tensor is 4 MB)
    ag = R.anchor_generator.AnchorGenerator(anchor_range=np.array(PC_RANGE, dtype=np.float32),
                                            anchor_generator_config=[dict(anchor_sizes=[[3.9, 1.6, 1.56]], anchor_rotations=[0, 1.57],
                                                                          anchor_bottom_heights=[-1.78], align_center=False)])
    anc, _ = ag.generate_anchors([np.array([296, 248])])
    a = anc[0].reshape(-1, 7).numpy()
    np.savez_compressed(os.path.join(OUT, "g5_anchors_full.npz"), shape=np.array(anc[0].shape), sample_idx=np.arange(0, a.shape[0], 97),
                        sample=a[::97], sum64=a.astype(np.float64).sum(0), x_row=anc[0][0, 0, :, 0, 0, 0].numpy(),
                        y_col=anc[0][0, :, 0, 0, 0, 1].numpy())


def g6_g7_coder(R):
    gen = torch.Generator().manual_seed(606)
    coder = R.box_coder_utils.ResidualCoder()
    anchors = torch.rand(64, 7, generator=gen) * 4 + 0.5
    boxes = torch.rand(64, 7, generator=gen) * 4 + 0.5
    enc = coder.encode_torch(boxes.clone(), anchors.clone())
    dec = coder.decode_torch(enc, anchors)
    val = torch.cat([torch.linspace(-10, 10, 401), torch.tensor([0.0, math_pi(), -math_pi(), 0.78539, 0.78539 + math_pi()])])
    np.savez_compressed(os.path.join(OUT, "g6_g7_coder.npz"), anchors=anchors.numpy(), boxes=boxes.numpy(), enc=enc.numpy(), dec=dec.numpy(),
                        lp_val=val.numpy(), lp_0_pi=R.common_utils.limit_period(val, 0.0, np.pi).numpy(),
                        lp_05_2pi=R.common_utils.limit_period(val, 0.5, 2 * np.pi).numpy(),
                        lp_0_2pi=R.common_utils.limit_period(val, 0.0, 2 * np.pi).numpy())


def math_pi():
    return float(np.pi)


def _head_cfg(stride=1):
    return EasyDict(
        CLASS_AGNOSTIC=False, USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
        ANCHOR_GENERATOR_CONFIG=[dict(class_name="Car", anchor_sizes=[[3.9, 1.6, 1.56]], anchor_rotations=[0, 1.57],
                                      anchor_bottom_heights=[-1.78], align_center=False, feature_map_stride=stride,
                                      matched_threshold=0.6, unmatched_threshold=0.45)],
        TARGET_ASSIGNER_CONFIG=dict(NAME="AxisAlignedTargetAssigner", POS_FRACTION=-1.0, SAMPLE_SIZE=512,
                                    NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False, BOX_CODER="ResidualCoder"),
        LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, mem_weight=1.0,
                                           code_weights=[1.0] * 7)))


def g8_assigner_losses(R):
    """Target assignment + the five losses of the training head on a small grid (reference code, CPU)."""
    gen = torch.Generator().manual_seed(808)
    nx, ny = 40, 32
    rng = np.array([0, -2.56, -2.5, 6.4, 2.56, 0.5], dtype=np.float32)     # 0.16 m cells
    torch.manual_seed(808)
    m = R.head_single.AnchorHeadSingle(model_cfg=_head_cfg(1), input_channels=24, num_class=1, class_names=["Car"],
                                       grid_size=np.array([nx, ny, 1]), point_cloud_range=rng)
    m.conv_box.weight.data.normal_(0, 0.05, generator=gen)
    m.conv_dir_cls.weight.data.normal_(0, 0.2, generator=gen)
    m.train()
    B, G = 2, 5
    gt = torch.zeros(B, G, 8)
    gt[0, 0] = torch.tensor([2.1, 0.3, -1.0, 3.9, 1.6, 1.56, 0.1, 1])
    gt[0, 1] = torch.tensor([4.8, -1.2, -1.0, 3.6, 1.5, 1.5, 1.45, 1])
    gt[0, 2] = torch.tensor([5.9, 2.2, -0.9, 4.2, 1.7, 1.6, -2.9, 1])
    gt[1, 0] = torch.tensor([3.3, -0.4, -1.1, 3.8, 1.6, 1.5, 0.8, 1])      # 45-degree-ish box: weak IoU with both anchors
    gt[1, 1] = torch.tensor([1.0, 1.9, -1.0, 4.0, 1.65, 1.55, 1.6, 1])
    f = torch.randn(B, 24, ny, nx, generator=gen)
    fp = torch.randn(B, 24, ny, nx, generator=gen)
    pos_p = torch.randn(37, 64, generator=gen)
    pos_m = torch.randn(37, 64, generator=gen)
    items = torch.randn(50, 64, generator=gen)
    d = m({"spatial_features_2d": f.clone(), "spatial_features_point_2d": fp.clone(), "point_positive_features": pos_p,
           "memory_positive_features": pos_m, "memory_items": items, "gt_boxes": gt.clone(), "batch_size": B})
    fr = m.forward_ret_dict
    targets = {k: fr[k].detach().clone().numpy() for k in ("box_cls_labels", "box_reg_targets", "reg_weights")}
    rpn, rpn_pt, mem, tb, _ = m.get_loss()
    np.savez_compressed(os.path.join(OUT, "g8_assigner_losses.npz"), nx=nx, ny=ny, point_cloud_range=rng, gt_boxes=gt.numpy(),
                        spatial_features_2d=f.numpy(), spatial_features_point_2d=fp.numpy(), pos_point=pos_p.numpy(),
                        pos_memory=pos_m.numpy(), rpn_loss=rpn.item(), rpn_loss_point=rpn_pt.item(), mem_loss=mem.item(),
                        **{"tb." + k: np.float64(v) for k, v in tb.items()}, **{"target." + k: v for k, v in targets.items()},
                        **{"param." + k: v for k, v in sd_np(m).items()})


G18_CLASSES = {
    # name -> (class names, per class: anchor size, bottom height, matched / unmatched threshold): hvpr.yaml's one-class head (the
    # _head_cfg of G8) and hvpr_3class.yaml's three anchor sets, as plain values
    "car": (["Car"], [[3.9, 1.6, 1.56]], [-1.78], [0.6], [0.45]),
    "3c": (["Car", "Pedestrian", "Cyclist"], [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], [-1.78, -0.6, -0.6],
           [0.6, 0.5, 0.5], [0.45, 0.35, 0.35]),
}
G18_ROTATIONS = [0, 1.57]
G18_PAD = 50                      # rows per frame of the mixed batch (the padded size hvpr.yaml's loader produces)


def _g18_head_cfg(which):
    names, sizes, heights, matched, unmatched = G18_CLASSES[which]
    cfg = _head_cfg(1)
    cfg.ANCHOR_GENERATOR_CONFIG = [dict(class_name=n, anchor_sizes=[s], anchor_rotations=list(G18_ROTATIONS), anchor_bottom_heights=[h],
                                        align_center=False, feature_map_stride=1, matched_threshold=m, unmatched_threshold=u)
                                   for n, s, h, m, u in zip(names, sizes, heights, matched, unmatched)]
    return cfg


def g18_frames(which, anchors, iou):
    """The edge frames of G18 as {name: (G, 8) float32}.  `anchors`: the head's anchor tensors (case 10 sits on anchor centres),
    `iou`: the reference's boxes3d_nearest_bev_iou.

    Rows whose trim outcome hinges on cancellation (`cancel*`) hold small dyadic numbers only — multiples of 0.25 below 16 — so
    that every partial sum of the 7 box fields is exact in fp32 in EVERY summation order: the reference sums on whatever device
    it runs on, in an order that is not ours to know, and the outcome `sum == 0` must not depend on it."""
    three = which == "3c"
    last = 3 if three else 1                                            # the class that class 0 wraps to (class_names[-1])
    car = [1.5, 1.0, -1.0, 4.0, 1.5, 1.5, 0.0, 1]
    ped = [2.0, 1.0, -0.5, 0.75, 0.5, 1.75, 0.25, 2]
    cyc = [4.5, -1.5, -0.5, 1.75, 0.5, 1.75, -0.5, 3]
    first = ped if three else car
    cancel = [3.0, -1.0, -1.0, 4.0, 1.5, 1.5, -8.0, 1]                   # a real car: 3 - 1 - 1 + 4 + 1.5 + 1.5 - 8 == 0
    moved = cancel[:6] + [-7.5, 1]                                       # the same car, heading moved by 0.5: the sum is 0.5
    zero = [0.0] * 8
    f = {}
    # 1. trailing real box whose signed 7-field sum is exactly 0: last row / followed by all-zero rows; the control keeps it
    f["cancel_last"] = [first, cancel]
    f["cancel_then_zeros"] = [first, cancel, zero, zero, zero]
    f["cancel_control_moved"] = [first, moved]
    f["cancel_inside"] = [first, cancel, cyc if three else car]          # not trailing: stays
    # 2. trailing row with a zero box and a non-zero class
    for c in ((1, 2, 3) if three else (1,)):
        f[f"zero_box_class{c}_trailing"] = [first, car, zero[:7] + [c]]
    # 3. all-zero row inside the valid range: class 0 wraps to the last class name
    f["zero_row_inside"] = [car, zero, cyc if three else cancel[:6] + [1.5, 1]]
    # 4. G = 1: cnt stops at 0, row 0 is never trimmed; one class entry -> the reference's other mask branch (:62-66)
    f["g1_all_zero"] = [zero]
    f[f"g1_zero_box_class{last}"] = [zero[:7] + [last]]
    f["g1_real"] = [car]
    # 5. only padding
    f["only_padding"] = [zero] * 4
    # 6. two identical ground truths: the first maximum wins.  Class 0 reads class_names[-1]: it shares the last class's anchor set
    #    with a real ground truth of that class, and whichever comes first gives the label (0 = no positive at all)
    box = cyc if three else car
    f["twins_same_class"] = [box, box]
    f["twins_real_first"] = [box, box[:7] + [0]]
    f["twins_class0_first"] = [box[:7] + [0], box]
    # 7. a ground truth that overlaps no anchor (no forced match, :155-156) next to one that does
    far = [30.0, 0.5, -1.0, 3.9, 1.6, 1.56, 0.3, 1]
    f["far_and_near"] = [far, car]
    f["near_only"] = [car]
    # 8. a ground truth that fits another class's anchors better than its own: the masks are per class
    if three:
        f["cyclist_sized_pedestrian"] = [[3.0, 0.5, -0.6, 1.76, 0.6, 1.73, 0.0, 2], [5.0, -1.0, -0.6, 0.8, 0.6, 1.73, 1.57, 3]]
    # 9. headings on the axis-snap border (|limit_period(r, 0.5, pi)| < pi/4) as fp32 and their fp32 neighbours on both sides
    for tag, base in (("pi4", np.pi / 4), ("mpi4", -np.pi / 4), ("3pi4", 3 * np.pi / 4)):
        b32 = np.float32(base)
        hs = [np.nextafter(b32, np.float32(-10)), b32, np.nextafter(b32, np.float32(10))]
        rows = []
        for h, y in zip(hs, (-1.6, 0.0, 1.6)):
            if three:
                rows.append([2.0, y, -0.6, 1.76, 0.6, 1.73, float(h), 3])
                rows.append([5.0, y, -0.6, 0.8, 0.6, 1.73, float(h), 2])
            else:
                rows.append([3.2, y, -1.0, 3.9, 1.6, 1.56, float(h), 1])
        f["snap_" + tag] = rows
    # 10. on an anchor centre.  (a) with the anchor's own box: IoU exactly 1 with the rotation-0 anchor — the other rotation of that
    #     location has the dimensions swapped, so with no square anchor in either head it does NOT tie.  (b) a SQUARE footprint
    #     inside both rotations' boxes: the two rotations of the location tie for the ground truth's maximum, both are forced.
    #     The areas of the two anchors are products of rounded extents about different centre coordinates and may differ in the last
    #     bit, so the cell is searched for: the first interior one where the reference's own IoU of both rotations is the maximum.
    k = 1 if three else 0
    a = anchors[k][0, 13, 17]                                           # (sizes, rotations, 7) at grid cell y 13, x 17
    f["on_anchor_exact"] = [a[0, 0].tolist() + [k + 1]]
    side = 0.4 if three else 1.0
    for cy, cx in ((y, x) for y in range(8, 24) for x in range(12, 28)):
        a = anchors[k][0, cy, cx, 0]                                    # (rotations, 7)
        sq = a[0].tolist() + [k + 1]
        sq[3] = sq[4] = side
        v = iou(anchors[k].reshape(-1, 7).clone(), torch.tensor([sq[:7]]))[:, 0].reshape(anchors[k].shape[1:5])[:, :, 0]
        if float(v[cy, cx, 0]) == float(v[cy, cx, 1]) == float(v.max()):
            break
    else:
        raise AssertionError("no cell where the two rotations tie")
    f["on_anchor_square"] = [sq]
    f["on_anchor_square_cell"] = (cy, cx)
    # 11. 50 random ground truths of all classes
    r = np.random.default_rng(1818)
    sizes = np.array(G18_CLASSES[which][1], np.float32)
    cls = r.integers(0, len(sizes), G18_PAD)
    g = np.zeros((G18_PAD, 8), np.float32)
    g[:, 0] = r.uniform(0.3, 6.1, G18_PAD)
    g[:, 1] = r.uniform(-2.3, 2.3, G18_PAD)
    g[:, 2] = r.uniform(-1.2, -0.6, G18_PAD)
    g[:, 3:6] = sizes[cls] * r.uniform(0.85, 1.15, (G18_PAD, 3))
    g[:, 6] = r.uniform(-np.pi, np.pi, G18_PAD)
    g[:, 7] = cls + 1
    f["random50"] = g
    cell = f.pop("on_anchor_square_cell")
    return {k: np.asarray(v, np.float32).reshape(-1, 8) for k, v in f.items()}, cell


def g18_assigner_edges(R):
    """G18: the reference's own AnchorHeadSingle.assign_targets (AxisAlignedTargetAssigner, CPU) on the 40 x 32 grid of G8 at the
    assigner's edges (g18_frames), for the one-class head of G8 and the three-class head of hvpr_3class.yaml.  Stored, data only:
    grid, range, the class configuration as plain values, every frame, and per frame the reference's box_cls_labels, reg_weights
    and box_reg_targets (the rows with label > 0 and their indices: every other row is exactly zero, asserted here).  Every frame
    padded with zero rows to 50 and stacked is one mixed batch; the reference gives for it, frame by frame, what it gives for the
    frames alone (asserted here), so the batch needs no data of its own."""
    nx, ny = 40, 32
    rng = np.array([0, -2.56, -2.5, 6.4, 2.56, 0.5], dtype=np.float32)     # 0.16 m cells, as G8
    out = dict(nx=nx, ny=ny, point_cloud_range=rng, anchor_rotations=np.array(G18_ROTATIONS, np.float64), pad_rows=G18_PAD,
               configs=np.array(list(G18_CLASSES)))
    for which, (names, sizes, heights, matched, unmatched) in G18_CLASSES.items():
        torch.manual_seed(1800)
        m = R.head_single.AnchorHeadSingle(model_cfg=_g18_head_cfg(which), input_channels=8, num_class=len(names), class_names=names,
                                           grid_size=np.array([nx, ny, 1]), point_cloud_range=rng)
        frames, (cy, cx) = g18_frames(which, m.anchors, R.box_utils.boxes3d_nearest_bev_iou)
        out.update({f"{which}.class_names": np.array(names), f"{which}.anchor_sizes": np.array(sizes, np.float64),
                    f"{which}.anchor_bottom_heights": np.array(heights, np.float64), f"{which}.matched": np.array(matched, np.float64),
                    f"{which}.unmatched": np.array(unmatched, np.float64), f"{which}.cases": np.array(list(frames))})
        res = {}
        for name, gt in frames.items():
            t = m.assign_targets(gt_boxes=torch.from_numpy(gt.copy())[None])
            lab, tgt, w = (t[k][0].numpy() for k in ("box_cls_labels", "box_reg_targets", "reg_weights"))
            pos = np.nonzero(lab > 0)[0]
            assert not tgt[lab <= 0].any() and np.isfinite(tgt).all() and lab.min() >= -1 and lab.max() <= len(names)
            res[name] = (lab, tgt, w)
            out.update({f"{which}.{name}.gt": gt, f"{which}.{name}.labels": lab.astype(np.int8), f"{which}.{name}.reg_weights": w,
                        f"{which}.{name}.pos_idx": pos.astype(np.int32), f"{which}.{name}.pos_targets": tgt[pos]})
        npos = {k: int((v[0] > 0).sum()) for k, v in res.items()}
        # the cases do what they are for
        assert npos["cancel_last"] < npos["cancel_control_moved"], npos                      # 1: the reference trims the cancelling row
        for k in ("labels", "pos_idx", "pos_targets"):
            assert np.array_equal(out[f"{which}.cancel_last.{k}"], out[f"{which}.cancel_then_zeros.{k}"])
        assert npos["cancel_inside"] > npos["cancel_last"]
        assert npos["only_padding"] == npos["g1_all_zero"] == 0 and npos["g1_real"] > 0
        assert npos["twins_real_first"] == npos["twins_same_class"] > 0 and npos["twins_class0_first"] == 0   # 6: first maximum
        assert np.array_equal(res["far_and_near"][0], res["near_only"][0]) and npos["near_only"] > 0          # 7: no positive from afar
        iou = R.box_utils.boxes3d_nearest_bev_iou
        k = 1 if which == "3c" else 0
        flat = m.anchors[k].reshape(-1, 7)
        assert float(iou(flat, torch.from_numpy(frames["on_anchor_exact"][:, :7].copy())).max()) == 1.0       # 10a: IoU exactly 1
        lab_sq = res["on_anchor_square"][0].reshape(ny, nx, -1)
        per_loc = (lab_sq > 0).sum(-1)
        assert per_loc[cy, cx] >= 2, per_loc[cy, cx]                                          # 10b: both rotations forced at one location
        v = iou(flat, torch.from_numpy(frames["on_anchor_square"][:, :7].copy()))[:, 0]
        thr = unmatched[k]
        assert float(v.max()) < thr and int((v == v.max()).sum()) == npos["on_anchor_square"]  # ... and ONLY forced: all below unmatched
        if which == "3c":
            lab8 = res["cyclist_sized_pedestrian"][0].reshape(ny, nx, 3, 2)
            assert set(np.unique(lab8[:, :, 1][lab8[:, :, 1] > 0])) == {2} and set(np.unique(lab8[:, :, 2][lab8[:, :, 2] > 0])) == {3}
            assert not (lab8[:, :, 0] > 0).any()                                             # 8: masks per class
        for tag in ("pi4", "mpi4", "3pi4"):
            assert npos["snap_" + tag] > 0
        assert npos["random50"] >= 25
        # the mixed batch: every frame padded to 50 rows; the reference treats frames independently
        batch = np.zeros((len(frames), G18_PAD, 8), np.float32)
        for i, gt in enumerate(frames.values()):
            batch[i, :len(gt)] = gt
        t = m.assign_targets(gt_boxes=torch.from_numpy(batch))
        for i, name in enumerate(frames):
            for k, v in zip(("box_cls_labels", "box_reg_targets", "reg_weights"), res[name]):
                assert np.array_equal(t[k][i].numpy(), v), (which, name, k)
        print(f"g18 {which}: positives per case", npos)
    np.savez_compressed(os.path.join(OUT, "g18_assigner_edges.npz"), **out)


def g9_onecycle(R):
    import collections
    import collections.abc
    collections.Iterable = collections.abc.Iterable           # fastai_optim.py:3 predates python 3.10
    fo = _load("tools_opt.fastai_optim", "tools/train_utils/optimization/fastai_optim.py")
    sys.modules["tools_opt"] = types.ModuleType("tools_opt"); sys.modules["tools_opt"].__path__ = []
    sys.modules["tools_opt.fastai_optim"] = fo
    ls = _load("tools_opt.learning_schedules_fastai", "tools/train_utils/optimization/learning_schedules_fastai.py")
    from functools import partial
    torch.manual_seed(909)
    net = torch.nn.Sequential(torch.nn.Linear(6, 5, bias=False), torch.nn.BatchNorm1d(5), torch.nn.ReLU(), torch.nn.Linear(5, 3))
    init = {k: v.detach().clone().numpy() for k, v in net.state_dict().items() if "num_batches" not in k}
    flat = lambda mm: sum(map(flat, mm.children()), []) if len(list(mm.children())) else [mm]
    opt = fo.OptimWrapper.create(partial(torch.optim.Adam, betas=(0.9, 0.99)), 3e-3, [torch.nn.Sequential(*flat(net))], wd=0.01,
                                 true_wd=True, bn_wd=True)
    sched = ls.OneCycle(opt, 100, 0.003, [0.95, 0.85], 10, 0.4)
    lrs, moms = [], []
    gen = torch.Generator().manual_seed(910)
    xs = torch.randn(3, 16, 6, generator=gen)
    after = []
    for it in range(100):
        sched.step(it)
        lrs.append(float(opt.lr)); moms.append(float(opt.mom))
        if it < 3:
            net.train(); opt.zero_grad()
            net(xs[it]).pow(2).mean().backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), 10)
            opt.step()
            after.append({k: v.detach().clone().numpy() for k, v in net.state_dict().items() if "num_batches" not in k})
    np.savez_compressed(os.path.join(OUT, "g9_onecycle.npz"), lr=np.array(lrs), mom=np.array(moms), x=xs.numpy(),
                        **{"init." + k: v for k, v in init.items()},
                        **{f"after{i}." + k: v for i, a in enumerate(after) for k, v in a.items()})


def g10_train_memory(R):
    gen = torch.Generator().manual_seed(1010)
    cfg = EasyDict(NUM_BEV_FEATURES=128, NUM_COORD_POINTS=3, NUM_PT_FEATURES=64, NUM_SCALE_FEATURES=32, NUM_K=20, NUM_M=2000,
                   SHRINK_TH=0.0025)
    m = R.scatter.PointPillarScatter_Agg_Memory_1_scale(model_cfg=cfg, grid_size=np.array([12, 10, 1]))
    load_det(m, 1010)
    m.train()
    pillars = torch.relu(torch.randn(60, 64, generator=gen))
    points = torch.relu(torch.randn(900, 64, generator=gen))
    with torch.no_grad():
        gs = m.get_score(points, pillars.t())
        score = torch.softmax(points @ pillars.t(), dim=0)
        idx = torch.topk(score, 20, dim=0)[1]
        positives = points[idx].permute(1, 0, 2).contiguous()
        mem = m.memory(pillars, 20, positives)
    np.savez_compressed(os.path.join(OUT, "g10_train_memory.npz"), pillars=pillars.numpy(), points=points.numpy(), W_seed=1010,
                        W_name="memory.weight", get_score_output=gs["output"].numpy(), positives=positives.numpy(),
                        memory_output=mem["output"].numpy(), memory_att_rowsum=mem["att"].sum(1).numpy(),
                        memory_att_nnz=(mem["att"] > 0).sum(1).numpy())


def g11_preprocess(R):
    """Point pre-processing: range mask, KITTI FOV flag, sample_points (reference code, numpy RNG seeded)."""
    import ast
    _stub("pcdet.datasets", os.path.join(REF, "pcdet/datasets"))
    _stub("pcdet.datasets.processor", os.path.join(REF, "pcdet/datasets/processor"))
    dp = _load("pcdet.datasets.processor.data_processor", "pcdet/datasets/processor/data_processor.py")
    calib_mod = _load("pcdet.utils.calibration_kitti", "pcdet/utils/calibration_kitti.py")
    # get_fov_flag lives in a module that imports the whole dataset stack: take the function's own source out of the file
    tree = ast.parse(open(os.path.join(REF, "pcdet/datasets/kitti/kitti_dataset.py")).read())
    fn = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "get_fov_flag"][0]
    fn.decorator_list = []
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "kitti_dataset.py", "exec"), ns)
    get_fov_flag = ns["get_fov_flag"]

    rng = np.random.default_rng(1111)
    n = 3000
    mix = np.where(rng.random((n - 8, 1)) < 0.8, rng.uniform([-10, -30, -3, 0], [36, 30, 1, 1], (n - 8, 4)),
                   rng.uniform([-10, -45, -3, 0], [80, 45, 1, 1], (n - 8, 4)))      # ~12 % beyond 40 m
    pts = np.concatenate([mix,
                          [[0, -39.68, 0, 0], [69.12, 39.68, 0, 0], [69.12001, 0, 0, 0], [-1e-6, 0, 0, 0], [0, 0, 0, 0],
                           [30, 0, -1, 0.5], [39.99, 0.5, 0.3, 0.1], [40.5, 1, -1, 0.2]]]).astype(np.float32)
    rngr = np.array([0, -39.68, -3, 69.12, 39.68, 1], np.float32)
    mask = R.common_utils.mask_points_by_range(pts, rngr)
    calib = {"P2": np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]], np.float32),
             "R0": np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459],
                             [0.007402527, 0.004351614, 0.9999631]], np.float32),
             "Tr_velo2cam": np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766],
                                      [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                                      [0.9998621, 0.00752379, 0.01480755, -0.2717806]], np.float32)}
    C = calib_mod.Calibration(calib)
    img_shape = np.array([375, 1242], np.int32)
    fov = get_fov_flag(C.lidar_to_rect(pts[:, 0:3]), img_shape, C)
    cases = {}
    proc = dp.DataProcessor([], rngr, training=False)
    for tag, m, num in (("down", 2500, 1024), ("down_more_far", 2500, 700), ("up", 700, 1024), ("same", 1024, 1024)):
        np.random.seed(7 + num + m)
        sub = pts[:m].copy()
        out = proc.sample_points({"points": sub.copy()}, config=EasyDict(NUM_POINTS={"train": num, "test": num}))["points"]
        cases[tag + "_in"] = sub
        cases[tag + "_out"] = out
        cases[tag + "_seed"] = np.int64(7 + num + m)
        cases[tag + "_num"] = np.int64(num)
    np.savez_compressed(os.path.join(OUT, "g11_preprocess.npz"), points=pts, range=rngr, range_mask=mask, fov=fov,
                        P2=calib["P2"], R0=calib["R0"], V2C=calib["Tr_velo2cam"], img_shape=img_shape, **cases)
    print("g11 ok: range keeps", int(mask.sum()), "fov keeps", int(fov.sum()))


def synthetic_kitti_annos(seed=1212, n_frames=24):
    """Small random KITTI-style annotation sets (camera frame): ground truth with all the ignore cases (Van, Person_sitting,
    DontCare, occlusion / truncation / height levels) and detections = jittered ground truth + false positives."""
    rng = np.random.default_rng(seed)
    names = ["Car", "Car", "Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare", "Truck"]
    dims_of = {"Car": (3.9, 1.56, 1.6), "Van": (5.0, 2.2, 1.9), "Pedestrian": (0.8, 1.73, 0.6), "Person_sitting": (0.8, 1.3, 0.6),
               "Cyclist": (1.76, 1.73, 0.6), "Truck": (8.0, 3.0, 2.5), "DontCare": (-1, -1, -1)}
    gts, dts = [], []

    def bbox_of(loc, dims):
        u = 620 + 720 * loc[0] / loc[2]
        v = 180 + 720 * (loc[1] - dims[1] / 2) / loc[2]
        hw, hh = 360 * max(dims[0], dims[2]) / loc[2], 360 * dims[1] / loc[2]
        return [u - hw, v - hh, u + hw, v + hh]
    for f in range(n_frames):
        n = int(rng.integers(2, 11)) if f != 3 else 0          # one frame without ground truth
        g = {k: [] for k in ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y")}
        d = {k: [] for k in ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")}
        for _ in range(n):
            nm = names[int(rng.integers(0, len(names)))]
            loc = np.array([rng.uniform(-12, 12), rng.uniform(1.4, 1.9), rng.uniform(6, 45)])
            dims = np.array(dims_of[nm]) * (rng.uniform(0.9, 1.1, 3) if nm != "DontCare" else 1)
            ry = rng.uniform(-np.pi, np.pi)
            bb = bbox_of(loc, np.abs(dims)) if nm != "DontCare" else [rng.uniform(0, 600), rng.uniform(100, 200), rng.uniform(650, 1200), rng.uniform(220, 370)]
            g["name"].append(nm); g["truncated"].append(rng.choice([0.0, 0.0, 0.0, 0.1, 0.2, 0.4, 0.6])); g["occluded"].append(int(rng.choice([0, 0, 0, 1, 2, 3])))
            g["alpha"].append(ry - np.arctan2(loc[0], loc[2])); g["bbox"].append(bb); g["dimensions"].append(dims); g["location"].append(loc)
            g["rotation_y"].append(ry)
            if nm not in ("DontCare",) and rng.random() < 0.85:      # a detection near this object, sometimes of another class
                j = rng.normal(0, 1, 3) * np.array([0.06, 0.02, 0.08]) * rng.choice([1, 1, 1, 4])
                dn = nm if rng.random() < 0.9 else "Car"
                dn = {"Van": "Car", "Person_sitting": "Pedestrian", "Truck": "Car"}.get(dn, dn)
                dd = dims * rng.uniform(0.97, 1.03, 3)
                dry = ry + rng.normal(0, 0.03) + (np.pi if rng.random() < 0.1 else 0)
                d["name"].append(dn); d["truncated"].append(0.0); d["occluded"].append(0); d["alpha"].append(dry - np.arctan2(loc[0] + j[0], loc[2] + j[2]))
                d["bbox"].append((np.array(bb) + rng.normal(0, 2, 4)).tolist()); d["dimensions"].append(dd); d["location"].append(loc + j)
                d["rotation_y"].append(dry); d["score"].append(float(np.round(rng.uniform(0.1, 1.0), 3)))
        for _ in range(int(rng.integers(0, 4))):               # false positives
            nm = ["Car", "Pedestrian", "Cyclist"][int(rng.integers(0, 3))]
            loc = np.array([rng.uniform(-12, 12), rng.uniform(1.4, 1.9), rng.uniform(6, 60)])
            dims = np.array(dims_of[nm]) * rng.uniform(0.9, 1.1, 3)
            ry = rng.uniform(-np.pi, np.pi)
            d["name"].append(nm); d["truncated"].append(0.0); d["occluded"].append(0); d["alpha"].append(ry - np.arctan2(loc[0], loc[2]))
            d["bbox"].append(bbox_of(loc, dims)); d["dimensions"].append(dims); d["location"].append(loc); d["rotation_y"].append(ry)
            d["score"].append(float(np.round(rng.uniform(0.1, 0.9), 3)))

        def pack(a, with_score):
            out = {"name": np.array(a["name"], dtype="<U16"), "truncated": np.array(a["truncated"], np.float64), "occluded": np.array(a["occluded"], np.int64),
                   "alpha": np.array(a["alpha"], np.float64), "bbox": np.array(a["bbox"], np.float64).reshape(-1, 4),
                   "dimensions": np.array(a["dimensions"], np.float64).reshape(-1, 3), "location": np.array(a["location"], np.float64).reshape(-1, 3),
                   "rotation_y": np.array(a["rotation_y"], np.float64)}
            if with_score:
                out["score"] = np.array(a["score"], np.float64)
            return out
        gts.append(pack(g, False)); dts.append(pack(d, True))
    return gts, dts


def g12_kitti_eval(R):
    """AP through the reference's eval.py, run as plain Python: numba.jit -> identity, the ABSENT rotate_iou.py -> a stub
    over the build's CPU rotated-intersection (oracle/iou3d_nms_ref.c, angle negated: rotation_y is clockwise in x-z).  Pins
    the evaluator's filtering / matching / PR / AP logic; the rotated intersection itself stays unpinned."""
    O = _import_oracle()

    def jit(*a, **k):
        return a[0] if (len(a) == 1 and callable(a[0]) and not k) else (lambda f: f)
    nb = _stub("numba"); nb.jit = jit; nb.prange = range

    def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
        def as7(b):
            t = np.zeros((len(b), 7), np.float32)
            t[:, 0:2], t[:, 3:5], t[:, 5], t[:, 6] = b[:, 0:2], b[:, 2:4], 1.0, -b[:, 4]
            return t
        inter = O.boxes_overlap_bev(as7(boxes), as7(query_boxes)).astype(np.float64) if len(boxes) and len(query_boxes) else \
            np.zeros((len(boxes), len(query_boxes)))
        a1, a2 = (boxes[:, 2] * boxes[:, 3])[:, None], (query_boxes[:, 2] * query_boxes[:, 3])[None, :]
        ua = {-1: a1 + a2 - inter, 0: a1 + 0 * a2, 1: a2 + 0 * a1}.get(criterion)
        return inter.astype(np.float32) if ua is None else np.where(inter > 0, inter / ua, 0.0).astype(np.float32)
    _stub("pcdet.datasets", os.path.join(REF, "pcdet/datasets"))
    _stub("pcdet.datasets.kitti", os.path.join(REF, "pcdet/datasets/kitti"))
    _stub("pcdet.datasets.kitti.kitti_object_eval_python", os.path.join(REF, "pcdet/datasets/kitti/kitti_object_eval_python"))
    _stub("pcdet.datasets.kitti.kitti_object_eval_python.rotate_iou").rotate_iou_gpu_eval = rotate_iou_gpu_eval
    ev = _load("pcdet.datasets.kitti.kitti_object_eval_python.eval", "pcdet/datasets/kitti/kitti_object_eval_python/eval.py")
    gts, dts = synthetic_kitti_annos()
    detail = {}
    text, ret = ev.get_official_eval_result(gts, dts, ["Car", "Pedestrian", "Cyclist"], PR_detail_dict=detail)
    keys = sorted(ret)
    np.savez_compressed(os.path.join(OUT, "g12_kitti_eval.npz"), keys=np.array(keys), values=np.array([ret[k] for k in keys], np.float64),
                        prec_bbox=detail["bbox"], prec_bev=detail["bev"], prec_3d=detail["3d"], prec_aos=detail["aos"], text=np.array(text))
    print("g12 ok:", {k: round(float(ret[k]), 3) for k in keys if "moderate" in k and "3d" in k})


def g13_voxel_index(R):
    """Voxel-id order + cap semantics through the reference's in-tree copy of the voxel index loop, tools/vis.py:9-60
    (`_points_to_bevmap_reverse_kernel` + its caller `points_to_bev` :63-107), executed as plain Python: numba.jit -> identity;
    only the top of the file is executed (imports of cv2 / matplotlib / the broken pcdet packages dropped, everything from
    `point_to_vis_bev` on — drawing helpers, the demo main — is not needed).  The loop is structurally identical to spconv's
    `points_to_voxel` (absent): fp32 floor((p - lo) / vs) :37, per-axis bounds test :38-40, zyx coordinate :41, first-touch
    `coor_to_voxelidx` map :44-50, `break` at max_voxels :47-48.  Saved per case: the points, and for every cell the loop
    opened its (z, y, x), its voxel id and the number of points the loop counted into it (bev_map[-1], :51)."""
    def jit(*a, **k):
        return a[0] if (len(a) == 1 and callable(a[0]) and not k) else (lambda f: f)
    nb = _stub("numba"); nb.jit = jit; nb.prange = range

    def head_only(src):
        lines = src.split("\n")
        stop = next(i for i, l in enumerate(lines) if l.startswith("def point_to_vis_bev"))
        keep = [l for l in lines[:stop] if not (l.startswith("import cv2") or l.startswith("import matplotlib") or l.startswith("from pcdet"))]
        return "\n".join(keep)
    vis = _load("hvpr_ref_tools_vis", "tools/vis.py", head_only)
    captured = {}
    kernel = vis._points_to_bevmap_reverse_kernel

    def spy(points, voxel_size, coors_range, coor_to_voxelidx, bev_map, height_lowers, with_reflectivity, max_voxels):
        kernel(points, voxel_size, coors_range, coor_to_voxelidx, bev_map, height_lowers, with_reflectivity, max_voxels)
        captured["map"], captured["bev"] = coor_to_voxelidx, bev_map
    vis._points_to_bevmap_reverse_kernel = spy
    rng = [0.0, -19.84, -2.5, 47.36, 19.84, 0.5]
    vs = [0.16, 0.16, 3.0]
    gen = np.random.default_rng(1313)
    out = {"range": np.array(rng, np.float32), "voxel_size": np.array(vs, np.float32)}
    for tag, n, max_voxels, spread in (("nocap", 4000, 40000, 1.0), ("cap", 4000, 700, 1.0), ("dense", 4000, 40000, 0.04), ("densecap", 4000, 40, 0.04), ("cap1", 300, 1, 1.0)):
        pts = np.empty((n, 4), np.float32)
        pts[:, 0] = gen.uniform(-1.0, 48.5, n) * spread + (10.0 if spread < 1 else 0.0)
        pts[:, 1] = gen.uniform(-21.0, 21.0, n) * spread
        pts[:, 2] = gen.uniform(-3.2, 1.0, n)
        pts[:, 3] = gen.uniform(0, 1, n)
        # exact borders: x == hi (dropped), x == lo (kept), y == +-hi, z == lo / hi, cell edges k * 0.16
        pts[:8, 0] = [47.36, 0.0, 47.359997, 0.16, 0.32, 0.48, 12.8, 25.6]
        pts[8:12, 1] = [-19.84, 19.84, 19.839998, 0.0]
        pts[12:14, 2] = [-2.5, 0.5]
        gen.shuffle(pts, axis=0)
        vis.points_to_bev(pts, vs, rng, max_voxels=max_voxels)
        cmap, bev = captured["map"], captured["bev"]
        z, y, x = np.nonzero(cmap >= 0)
        ids = cmap[z, y, x]
        order = np.argsort(ids)
        assert (ids[order] == np.arange(len(ids))).all()
        out[tag + "_points"] = pts
        out[tag + "_max_voxels"] = np.int32(max_voxels)
        out[tag + "_cells_zyx"] = np.stack([z, y, x], 1)[order].astype(np.int32)          # row v = cell of voxel id v
        out[tag + "_counts"] = bev[-1][y, x][order].astype(np.int32)                        # points the loop put into voxel v
        print("g13", tag, "voxels", len(ids), "max count", int(out[tag + "_counts"].max()))
    np.savez_compressed(os.path.join(OUT, "g13_voxel_index.npz"), **out)


def g14_axis_aligned_iou(R):
    """Partial pin of row a8 (the rotated-IoU sources are absent): for boxes whose heading is a multiple of pi/2 the rotated BEV
    IoU IS the axis-aligned IoU, which the reference does ship — box_utils.boxes3d_nearest_bev_iou (box_utils.py:297-323, the
    matcher of axis_aligned_target_assigner.py:146) on top of boxes_iou_normal (:252-272).  Stored: the boxes and the reference's
    IoU matrices; the test derives greedy-NMS survivors from the reference matrix and compares the oracle's / kernel's NMS."""
    gen = torch.Generator().manual_seed(1414)

    def boxes(n):
        b = torch.zeros(n, 7)
        b[:, 0] = torch.rand(n, generator=gen) * 12
        b[:, 1] = torch.rand(n, generator=gen) * 8 - 4
        b[:, 2] = torch.rand(n, generator=gen) - 1.5
        b[:, 3] = 3.0 + torch.rand(n, generator=gen) * 1.5
        b[:, 4] = 1.4 + torch.rand(n, generator=gen) * 0.5
        b[:, 5] = 1.4 + torch.rand(n, generator=gen) * 0.3
        b[:, 6] = torch.randint(-2, 3, (n,), generator=gen).float() * (np.pi / 2)
        return b
    a, b = boxes(48), boxes(40)
    b[0] = a[0]                                    # identical pair -> IoU 1
    b[1] = a[1]; b[1, 6] = a[1, 6] + np.pi         # same rectangle, opposite heading
    b[2] = a[2]; b[2, 0] += 50                     # far apart -> 0
    b[3] = a[3]; b[3, 3:5] = a[3, 3:5] * 0.5       # contained
    b[4] = a[4]; b[4, 6] = 0.0; a[4, 6] = np.pi / 2   # the same centre, crossed
    iou_ab = R.box_utils.boxes3d_nearest_bev_iou(a, b)
    # a dense cluster for NMS: 256 boxes around a few centres, scores distinct
    n = 256
    c = boxes(n)
    centres = torch.rand(12, 2, generator=gen) * torch.tensor([12.0, 8.0]) - torch.tensor([0.0, 4.0])
    c[:, 0:2] = centres[torch.randint(0, 12, (n,), generator=gen)] + torch.randn(n, 2, generator=gen) * 0.6
    scores = torch.rand(n, generator=gen)
    iou_cc = R.box_utils.boxes3d_nearest_bev_iou(c, c)
    np.savez_compressed(os.path.join(OUT, "g14_axis_aligned_iou.npz"), boxes_a=a.numpy(), boxes_b=b.numpy(), iou_ab=iou_ab.numpy(),
                        nms_boxes=c.numpy(), nms_scores=scores.numpy(), iou_nms=iou_cc.numpy())


def load_post_processing(R):
    """The reference's post-processing wrapper — model_nms_utils.py:6-65 and Detector3DTemplate.post_processing /
    generate_recall_record (detector3d_template.py:168-318) — imported as they are.  What is ABSENT from the reference is the
    native module they call, pcdet/ops/iou3d_nms (setup.py:53-62): `nms_gpu` and `boxes_iou3d_gpu` are stood in by thin
    wrappers over the CPU oracle's C routines, written from the upstream signature (sort descending, optional
    pre_maxsize cut, mask + sweep, `order[keep]`).  detector3d_template.py's package-relative imports of the module zoo
    (backbones, heads, transformer ...; none is used by the two methods) are dropped."""
    O = _import_oracle()
    iou = sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_utils"]

    def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
        order = scores.sort(0, descending=True)[1]
        if pre_maxsize is not None:
            order = order[:pre_maxsize]
        b = np.ascontiguousarray(boxes[order].numpy()[:, :7], dtype=np.float32)
        keep = O.nms_sorted(b, float(thresh))
        return order[torch.from_numpy(keep)].contiguous(), None

    def boxes_iou3d_gpu(boxes_a, boxes_b):
        return torch.from_numpy(O.boxes_iou3d(boxes_a.numpy(), boxes_b.numpy()))
    iou.nms_gpu, iou.boxes_iou3d_gpu = nms_gpu, boxes_iou3d_gpu
    _stub("pcdet.models.model_utils", os.path.join(REF, "pcdet/models/model_utils"))
    _stub("pcdet.models.detectors", os.path.join(REF, "pcdet/models/detectors"))
    R.model_nms_utils = _load("pcdet.models.model_utils.model_nms_utils", "pcdet/models/model_utils/model_nms_utils.py")

    def drop_zoo(src):
        lines = src.split("\n")
        assert lines[5].startswith("from ...ops.iou3d_nms") and lines[9].startswith("from ..model_utils")
        return "\n".join(l for i, l in enumerate(lines) if not (5 <= i <= 9))
    R.det_template = _load("pcdet.models.detectors.detector3d_template", "pcdet/models/detectors/detector3d_template.py", drop_zoo)
    R.det_template.iou3d_nms_utils = iou
    R.det_template.model_nms_utils = R.model_nms_utils
    return R


def _detection_like(gen, B, N, C, frac_pass, n_centres, logit_lo=-7.0, logit_hi=3.0):
    """Logits (B, N, C) with well separated distinct values (a shuffled grid: sigmoid on another device cannot reorder them or
    move one across SCORE_THRESH) and car-sized boxes clustered round a few centres so that NMS has work to do."""
    boxes = torch.zeros(B, N, 7)
    cls = torch.empty(B, N, C)
    thr_logit = float(np.log(0.1 / 0.9))
    for b in range(B):
        centres = torch.rand(n_centres, 2, generator=gen) * torch.tensor([44.0, 36.0]) + torch.tensor([1.5, -18.0])
        boxes[b, :, 0:2] = centres[torch.randint(0, n_centres, (N,), generator=gen)] + torch.randn(N, 2, generator=gen) * 0.7
        boxes[b, :, 2] = torch.randn(N, generator=gen) * 0.2 - 1.0
        boxes[b, :, 3:6] = torch.tensor([3.9, 1.6, 1.56]) * (0.8 + 0.4 * torch.rand(N, 3, generator=gen))
        boxes[b, :, 6] = (torch.rand(N, generator=gen) * 2 - 1) * np.pi
        n_pass = int(round(N * C * frac_pass[b]))
        hi = torch.linspace(thr_logit + 0.05, logit_hi, max(n_pass, 1))[:n_pass]
        lo = torch.linspace(logit_lo, thr_logit - 0.05, N * C - n_pass)
        v = torch.cat([hi, lo])
        cls[b] = v[torch.randperm(N * C, generator=gen)].view(N, C)
    return cls, boxes


def _gt_from(boxes_b, picks, shifts, G, labels):
    """gt_boxes rows (G, 8): copies of predicted boxes moved by `shifts` metres along x; the rest zero rows (collate padding)."""
    gt = torch.zeros(G, 8)
    for r, (i, dx, lab) in enumerate(zip(picks, shifts, labels)):
        gt[r, :7] = boxes_b[i]
        gt[r, 0] += dx
        gt[r, 7] = lab
    return gt


def g15_post_processing(R):
    """Row a8's WRAPPER pinned on the reference's own code: score mask -> top-k -> NMS keep -> index map -> labels -> recall
    counters, for the class-agnostic branch (one class and three classes, raw-score output), the MULTI_CLASSES_NMS branch, and
    the two functions of model_nms_utils.py called directly.  Frames: more candidates than NMS_PRE_MAXSIZE, fewer, none at all,
    more survivors than NMS_POST_MAXSIZE; gt_boxes with trailing zero rows, a zero row in the middle, and all rows zero (the
    reference's `while k > 0` then keeps ONE zero row as a ground truth: detector3d_template.py:290-293).

    Score ties: torch.topk / torch.sort leave the order of equal scores unspecified (it differs between CPU and GPU builds of
    torch), so the tie frames are built so that the reference's result does not depend on it as a SET — tied boxes far from
    everything (all survive), tied boxes under one stronger box (all suppressed), none straddling the NMS_PRE_MAXSIZE cut —
    and the tests compare after ordering equal scores by ascending id, the tie rule this build defines."""
    R = load_post_processing(R)
    gen = torch.Generator().manual_seed(1515)
    out = {}

    class _DS:
        class_names = ["Car"]

    def detector(num_class, multi, raw, pre, post, nms_thresh):
        cfg = EasyDict(POST_PROCESSING=dict(RECALL_THRESH_LIST=[0.3, 0.5, 0.7], SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=raw,
                                            EVAL_METRIC="kitti",
                                            NMS_CONFIG=dict(MULTI_CLASSES_NMS=multi, NMS_TYPE="nms_gpu", NMS_THRESH=nms_thresh,
                                                            NMS_PRE_MAXSIZE=pre, NMS_POST_MAXSIZE=post)))
        ds = _DS(); ds.class_names = ["Car", "Pedestrian", "Cyclist"][:num_class]
        return R.det_template.Detector3DTemplate(cfg, num_class, ds), cfg

    def run(tag, cls, boxes, gt, num_class, multi=False, raw=False, normalized=False, pre=512, post=60, nms_thresh=0.1):
        det, cfg = detector(num_class, multi, raw, pre, post, nms_thresh)
        B = cls.shape[0]
        bd = {"batch_size": B, "batch_box_preds": boxes.clone(), "cls_preds_normalized": normalized, "gt_boxes": gt.clone()}
        if multi:       # the reference's tensor form trips its own assert (label mapping arange(1, num_class) is one short,
            bd["batch_cls_preds"] = [cls.clone()]           # :219-224); the multi-head LIST form with a full mapping runs
            bd["multihead_label_mapping"] = [torch.arange(1, num_class + 1)]
        else:
            bd["batch_cls_preds"] = cls.clone()
        preds, recall, _ = det.post_processing(bd)
        out[tag + ".cls"], out[tag + ".boxes"], out[tag + ".gt_boxes"] = cls.numpy().copy(), boxes.numpy().copy(), gt.numpy().copy()
        out[tag + ".cfg"] = np.array([num_class, int(multi), int(raw), int(normalized), pre, post], np.int64)
        out[tag + ".nms_thresh"] = np.float32(nms_thresh)
        for b, p in enumerate(preds):
            out[f"{tag}.f{b}.pred_boxes"] = p["pred_boxes"].numpy()
            out[f"{tag}.f{b}.pred_scores"] = p["pred_scores"].numpy()
            out[f"{tag}.f{b}.pred_labels"] = p["pred_labels"].numpy().astype(np.int64)
        keys = sorted(recall)
        out[tag + ".recall_keys"] = np.array(keys)
        out[tag + ".recall_values"] = np.array([recall[k] for k in keys], np.int64)
        # no recalled-count may hang on round-off: every best IoU stays clear of the thresholds
        for b, p in enumerate(preds):
            g = gt[b]; k = len(g) - 1
            while k > 0 and g[k].sum() == 0:
                k -= 1
            if p["pred_boxes"].shape[0]:
                best = R.det_template.iou3d_nms_utils.boxes_iou3d_gpu(p["pred_boxes"][:, :7], g[:k + 1, :7]).max(0)[0]
                assert all((best - t).abs().min() > 5e-3 for t in (0.3, 0.5, 0.7)), (tag, b, best)
        # the two functions of model_nms_utils.py, called directly on the same frames
        ncfg = cfg.POST_PROCESSING.NMS_CONFIG
        for b in range(B):
            sc = cls[b] if normalized else torch.sigmoid(cls[b])
            if multi:
                s, l, bx = R.model_nms_utils.multi_classes_nms(sc, boxes[b], ncfg, score_thresh=0.1)
                out[f"{tag}.f{b}.mc_scores"], out[f"{tag}.f{b}.mc_labels"], out[f"{tag}.f{b}.mc_boxes"] = s.numpy(), l.numpy(), bx.numpy()
            else:
                sel, ss = R.model_nms_utils.class_agnostic_nms(sc.max(-1)[0], boxes[b], ncfg, score_thresh=0.1)
                sel = sel if torch.is_tensor(sel) else torch.zeros(0, dtype=torch.long)
                out[f"{tag}.f{b}.selected"] = sel.numpy().astype(np.int64)
                out[f"{tag}.f{b}.selected_scores"] = ss.numpy()
        print("g15", tag, "kept per frame", [len(p["pred_scores"]) for p in preds], dict(recall))

    def plant_ties(cls, boxes, b, n_pass_expected):
        """Frame b: (i) five boxes with one score, far from everything and from each other -> all survive; (ii) four boxes with
        one score stacked under a box with a higher score -> all suppressed.  Both groups sit well inside the top-k cut."""
        N = cls.shape[1]
        top = torch.sort(cls[b, :, 0], descending=True)[1]
        assert n_pass_expected > 40
        loners, under, boss = top[10:15], top[20:24], top[2]
        cls[b, loners, 0] = float(cls[b, top[10], 0])
        for j, i in enumerate(loners):
            boxes[b, i, 0], boxes[b, i, 1] = 100.0 + 12.0 * j, 60.0
        cls[b, under, 0] = float(cls[b, top[20], 0])
        boxes[b, boss, 0], boxes[b, boss, 1] = 200.0, -60.0
        for j, i in enumerate(under):
            boxes[b, i] = boxes[b, boss].clone()
            boxes[b, i, 0] += 0.05 * (j + 1)
        return loners, under

    # --- one class, class-agnostic (hvpr_car): > PRE candidates | < PRE | none | ties + > POST survivors
    N = 3000
    cls, boxes = _detection_like(gen, 4, N, 1, [0.5, 0.06, 0.0, 0.3], 40)
    boxes[3, :, 0:2] = torch.rand(N, 2, generator=gen) * torch.tensor([46.0, 38.0]) + torch.tensor([0.5, -19.0])   # spread: many survivors
    plant_ties(cls, boxes, 3, 900)
    order = [torch.sort(cls[b, :, 0], descending=True)[1] for b in range(4)]
    gt = torch.stack([
        _gt_from(boxes[0], order[0][[0, 5, 9, 14]].tolist(), [0.1, 0.8, 1.5, 30.0], 6, [1, 1, 1, 1]),
        _gt_from(boxes[1], order[1][[0, 1, 2, 3, 4, 6]].tolist(), [0.0, 0.3, 0.6, 0.9, 1.3, 2.5], 6, [1] * 6),
        torch.zeros(6, 8),
        _gt_from(boxes[3], order[3][[0, 1, 3]].tolist(), [0.2, 0.5, 1.1], 6, [1, 1, 1])])
    gt[3, 4] = gt[3, 2]; gt[3, 2] = 0            # a zero row in the MIDDLE stays a ground truth; only trailing ones are cut
    run("car", cls, boxes, gt, 1)
    run("car_normalized_raw", torch.sigmoid(cls), boxes, gt, 1, raw=True, normalized=True, pre=300, post=25, nms_thresh=0.25)

    # --- the yaml's own sizes (NMS_PRE_MAXSIZE 4096, NMS_POST_MAXSIZE 500, thresh 0.1 as in tools/cfgs/kitti_models/hvpr.yaml)
    cls, boxes = _detection_like(gen, 1, 7000, 1, [0.7], 400)
    boxes[0, :, 0:2] = torch.rand(7000, 2, generator=gen) * torch.tensor([46.0, 38.0]) + torch.tensor([0.5, -19.0])
    o = torch.sort(cls[0, :, 0], descending=True)[1]
    gt = _gt_from(boxes[0], o[[0, 3, 8]].tolist(), [0.0, 0.4, 1.3], 5, [1, 1, 1])[None]
    run("car_yaml_sizes", cls, boxes, gt, 1, pre=4096, post=500, nms_thresh=0.1)

    # --- three classes, class-agnostic branch: label = argmax + 1 (:241-247); once with raw scores out (:254-256)
    cls, boxes = _detection_like(gen, 2, 1500, 3, [0.2, 0.02], 30)
    o = [torch.sort(cls[b].max(-1)[0], descending=True)[1] for b in range(2)]
    gt = torch.stack([_gt_from(boxes[0], o[0][[0, 2, 4, 7, 11]].tolist(), [0.0, 0.4, 0.9, 1.4, 2.2], 7, [1, 2, 3, 1, 2]),
                      _gt_from(boxes[1], o[1][[0, 1]].tolist(), [0.3, 1.0], 7, [3, 1])])
    run("three_agnostic", cls, boxes, gt, 3, pre=256, post=40)
    run("three_agnostic_raw", cls, boxes, gt, 3, raw=True, pre=256, post=40)

    # --- three classes, MULTI_CLASSES_NMS branch (:214-239, model_nms_utils.py:28-65); frame 1: one class has no candidate
    cls[1, :, 1] = cls[1, :, 1].clamp(max=-3.0)
    run("three_multi", cls, boxes, gt, 3, multi=True, pre=200, post=30, nms_thresh=0.2)
    np.savez_compressed(os.path.join(OUT, "g15_post_processing.npz"), **out)


def g16_train_branch_gradients(R):
    """G16: which tensor receives which gradient in the training branch — the reference's own
    PointPillarScatter_Agg_Memory_1_scale.forward (pointpillar_scatter.py:87-167, get_score :67-83), MemoryUnit_Agg training
    branch (memory_module.py:31-59), AnchorHeadSingle training forward (anchor_head_single.py:41-108) and get_loss
    (anchor_head_template.py:262-291), CPU, fp32 and float64.

    T1 is patched in exactly as DESIGN.md decided, and nothing else: get_score additionally returns the k
    positive point features it already computes (:76), and the training branch hands them to the memory as its second input
    (`self.memory(pillars.t(), self.k)` at :133 has one argument too few for memory_module.py:29-34).

    The head is fed the canvases directly (128 input channels; the backbone between them is pinned by G4-train), so the stored
    scalars are the three losses of get_loss, and a fixed cotangent on the scale canvas gives that stream a gradient too:
        L = rpn_loss + rpn_loss_point + mem_loss + sum(spatial_scale_features * cot_scale).
    Stored: the three canvases, point / memory positive features, the losses (fp32 module), and from the float64 module the
    gradient of EACH loss separately w.r.t. pillar_features, point_features and memory.weight (an exactly-zero block = a
    `.detach()` of the reference: :76,:80,:140, memory_module.py:56, anchor_head_template.py:268), the gradient of L w.r.t.
    pillar_scale_features and every head parameter, and the norm-wise distance of the fp32 module's gradients from them."""
    import copy

    def patch_t1(src):
        a = "return {'output': output, 'att': score}"
        b = "points_memory = self.memory(pillars.t(), self.k)"
        assert src.count(a) == 1 and src.count(b) == 2          # the first occurrence is the training branch (:133), the second eval (:200)
        src = src.replace(a, "return {'output': output, 'att': score, 'positive': points_positive}")
        return src.replace(b, "points_memory = self.memory(pillars.t(), self.k, points_positive_['positive'])", 1)

    sc_mod = _load("pcdet.models.backbones_2d.map_to_bev.pointpillar_scatter_t1",
                   "pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py", patch_t1)
    seed = 1616
    gen = torch.Generator().manual_seed(seed)
    nx, ny, B = 12, 10, 2
    rng = np.array([0, -2.5, -2.5, 6.0, 2.5, 0.5], dtype=np.float32)                # 0.5 m cells
    cfg = EasyDict(NUM_BEV_FEATURES=128, NUM_COORD_POINTS=3, NUM_PT_FEATURES=64, NUM_SCALE_FEATURES=32, NUM_K=20, NUM_M=2000,
                   SHRINK_TH=0.0025)
    scat = sc_mod.PointPillarScatter_Agg_Memory_1_scale(model_cfg=cfg, grid_size=np.array([nx, ny, 1]))
    # the bank at 4x its initial range: with U(+-1/8) rows and post-ReLU features every softmax value stays below SHRINK_TH and
    # the addressing is identically zero (G10's regime); here 30-80 items per row pass the threshold
    W = det_state({"memory.weight": (2000, 64)}, seed)["memory.weight"] * 4.0
    scat.memory.weight.data = torch.from_numpy(W)
    scat.train()
    torch.manual_seed(seed)
    head = R.head_single.AnchorHeadSingle(model_cfg=_head_cfg(1), input_channels=128, num_class=1, class_names=["Car"],
                                          grid_size=np.array([nx, ny, 1]), point_cloud_range=rng)
    head.conv_cls.weight.data.normal_(0, 0.05, generator=gen)
    head.conv_box.weight.data.normal_(0, 0.05, generator=gen)
    head.conv_dir_cls.weight.data.normal_(0, 0.1, generator=gen)
    head.conv_box.bias.data.normal_(0, 0.1, generator=gen)
    head.train()
    M = [57, 63]
    N = [900, 860]
    cells = [torch.randperm(nx * ny, generator=gen)[:m] for m in M]
    coords = torch.cat([torch.stack([torch.full((m,), b), torch.zeros(m, dtype=torch.long), c // nx, c % nx], dim=1)
                        for b, (m, c) in enumerate(zip(M, cells))]).float()
    pillars = torch.relu(torch.randn(sum(M), 64, generator=gen))
    scale = torch.relu(torch.randn(sum(M), 32, generator=gen))
    points = torch.relu(torch.randn(sum(N), 64, generator=gen)) * 0.5
    point_coords = torch.cat([torch.cat([torch.full((n, 1), float(b)), torch.rand(n, 3, generator=gen)], dim=1) for b, n in enumerate(N)])
    gt = torch.zeros(B, 4, 8)
    gt[0, 0] = torch.tensor([2.2, 0.3, -1.0, 3.9, 1.6, 1.56, 0.1, 1])
    gt[0, 1] = torch.tensor([4.1, -1.4, -1.0, 3.6, 1.5, 1.5, 1.45, 1])
    gt[1, 0] = torch.tensor([3.3, -0.4, -1.1, 3.8, 1.6, 1.5, 0.8, 1])
    gt[1, 1] = torch.tensor([1.4, 1.5, -1.0, 4.0, 1.65, 1.55, 1.6, 1])
    gt[1, 2] = torch.tensor([5.0, 0.9, -0.9, 4.2, 1.7, 1.6, -2.9, 1])
    cot = torch.from_numpy(det_state({"cotangent.scale": (B, 32, ny, nx)}, seed)["cotangent.scale"]) * 0.01
    res = {}
    for dt in (torch.float32, torch.float64):
        s, h = copy.deepcopy(scat).to(dt), copy.deepcopy(head).to(dt)
        h.anchors = [a.to(dt) for a in h.anchors]
        ins = {k: v.clone().to(dt).requires_grad_(True) for k, v in (("pillar_features", pillars), ("point_features", points),
                                                                      ("pillar_scale_features", scale))}
        d = s({**ins, "pillar_mask": torch.ones(sum(M), 32, 1, dtype=dt), "voxel_coords": coords.to(dt),
               "point_coords": point_coords.to(dt)})
        canv = {k: d[k] for k in ("spatial_features", "spatial_features_point", "spatial_scale_features")}
        d.update(spatial_features_2d=d["spatial_features"], spatial_features_point_2d=d["spatial_features_point"],
                 gt_boxes=gt.clone().to(dt), batch_size=B)
        h(d)
        rpn, rpn_pt, mem, tb, items = h.get_loss()
        assert items is s.memory.weight
        leaves = [ins["pillar_features"], ins["point_features"], s.memory.weight]
        per = {}
        for name, val in (("rpn_loss", rpn), ("rpn_loss_point", rpn_pt), ("mem_loss", mem)):
            g = torch.autograd.grad(val, leaves, retain_graph=True, allow_unused=True)
            per[name] = [torch.zeros_like(l) if x is None else x for x, l in zip(g, leaves)]
        total = rpn + rpn_pt + mem + (canv["spatial_scale_features"] * cot.to(dt)).sum()
        hp = dict(h.named_parameters())
        g = torch.autograd.grad(total, [ins["pillar_scale_features"]] + list(hp.values()))
        res[dt] = dict(canv={k: v.detach() for k, v in canv.items()}, pos_point=d["point_positive_features"].detach(),
                       pos_mem=d["memory_positive_features"].detach(), losses=(rpn.item(), rpn_pt.item(), mem.item()),
                       tb={k: float(v) for k, v in tb.items()}, per=per, gscale=g[0], ghead=dict(zip(hp.keys(), g[1:])),
                       labels=h.forward_ret_dict["box_cls_labels"].detach())
    r32, r64 = res[torch.float32], res[torch.float64]

    def nerr(a, b):
        return float((a.double() - b).norm() / b.norm().clamp_min(1e-300))
    out = dict(nx=nx, ny=ny, point_cloud_range=rng, seed=seed, bank_scale=4.0, pillar_features=pillars.numpy(),
               pillar_scale_features=scale.numpy(), point_features=points.numpy(), voxel_coords=coords.numpy(),
               point_coords=point_coords.numpy(), gt_boxes=gt.numpy(), cot_scale=cot.numpy(),
               box_cls_labels=r32["labels"].numpy(), losses=np.array(r32["losses"], dtype=np.float64),
               losses_f64=np.array(r64["losses"], dtype=np.float64), point_positive_features=r32["pos_point"].numpy(),
               memory_positive_features=r32["pos_mem"].numpy(),
               memory_positive_features_f64=r64["pos_mem"].float().numpy())
    for k, v in r32["canv"].items():
        out[k] = v.numpy()
    for k, v in r32["tb"].items():
        out["tb." + k] = np.float64(v)
    for k, v in sd_np(head).items():
        out["param." + k] = v
    for loss in ("rpn_loss", "rpn_loss_point", "mem_loss"):
        for name, g32, g64 in zip(("pillar_features", "point_features", "memory.weight"), r32["per"][loss], r64["per"][loss]):
            key = f"{loss}.{name}"
            if float(g64.abs().max()) == 0.0:
                assert float(g32.abs().max()) == 0.0
                out["zero." + key] = True                          # a detach of the reference: exactly no gradient
            else:
                out["zero." + key] = False
                out["grad." + key] = g64.float().numpy()
                out["ref32_err." + key] = nerr(g32, g64)
    out["grad.total.pillar_scale_features"] = r64["gscale"].float().numpy()
    out["ref32_err.total.pillar_scale_features"] = nerr(r32["gscale"], r64["gscale"])
    for k, g64 in r64["ghead"].items():
        out["grad.total.head." + k] = g64.float().numpy()
        out["ref32_err.total.head." + k] = nerr(r32["ghead"][k], g64)
    np.savez_compressed(os.path.join(OUT, "g16_train_branch_gradients.npz"), **out)
    return out


def g17_stubs(log):
    """Recording stand-ins for everything train_one_epoch is handed: (model, optimizer, lr_scheduler, tbar, model_func, clip, items,
    loader).  Every call appends one line to `log`.  Shared with tests/train_fixture_cases.py, which drives the SAME stand-ins with
    its own loop and must produce the same lines."""
    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(3))

        def train(self, mode=True):
            log.append(f"model.train({mode})" if mode is not True else "model.train()")
            return super().train(mode)

        def parameters(self, recurse=True):
            log.append("model.parameters()")
            return super().parameters(recurse)

    class Optimizer:
        def __init__(self):
            self._lr = 0.0

        @property
        def lr(self):
            log.append("read optimizer.lr")
            return self._lr

        def zero_grad(self):
            log.append("optimizer.zero_grad()")

        def step(self):
            log.append("optimizer.step()")

    class Scheduler:
        def __init__(self, opt):
            self.opt = opt

        def step(self, it):
            log.append(f"lr_scheduler.step({it})")
            self.opt._lr = 0.001 * (it + 1)

    class Bar:
        def set_postfix(self, d):
            log.append("tbar.set_postfix(" + ", ".join(f"{k}:{type(v).__name__}" for k, v in d.items()) + ")")

        def refresh(self):
            log.append("tbar.refresh()")

    model, opt = Model(), Optimizer()
    items = torch.arange(6.0).view(3, 2)

    def model_func(m, batch):
        assert m is model
        log.append(f"model_func(model, batch[{batch['id']}])")
        loss = (m.w * float(batch["id"] + 1)).sum()
        loss.register_hook(lambda g: log.append("loss.backward()"))
        return loss, {"tb_scalar": 1.5}, {"disp_scalar": 2.5}, items

    def clip(params, max_norm):
        params = list(params)
        log.append(f"clip_grad_norm_(<{len(params)} parameters of the model>, {max_norm})")
        assert params[0] is model.w and model.w.grad is not None
    return model, opt, Scheduler(opt), Bar(), model_func, clip, items, [{"id": i} for i in range(3)]


def g17_train_loop_protocol(R):
    """G17: the call protocol of the reference's training loop — tools/train_utils/train_utils.py:9-61 `train_one_epoch` run as it
    is, with recording stand-ins (g17_stubs) for everything it is handed (model, optimizer, lr_scheduler, model_func, the data
    loader, tbar) and for the `clip_grad_norm_` it imports.  Stored: the sequence of calls with their arguments for 3 iterations
    starting at accumulated_iter = 7, what it returns, and what it puts into the progress bar.  The plugin objects of the product
    (model_fn_decorator, FusedAdamOneCycle, OneCycle) must work when driven in exactly this order."""
    tu = _load("tools_train_utils_g17", "tools/train_utils/train_utils.py")
    log = []
    model, opt, sched, bar, model_func, clip, items, loader = g17_stubs(log)
    tu.clip_grad_norm_ = clip
    cfg = EasyDict(GRAD_NORM_CLIP=10)
    ret_it, ret_items = tu.train_one_epoch(model, opt, loader, model_func, sched, accumulated_iter=7, optim_cfg=cfg, rank=0,
                                           tbar=bar, total_it_each_epoch=3, dataloader_iter=iter(loader), tb_log=None, leave_pbar=False)
    assert ret_items is items
    np.savez_compressed(os.path.join(OUT, "g17_train_loop_protocol.npz"), calls=np.array(log), start_iter=7, n_iters=3,
                        returned_iter=ret_it, returns_items_of_last_model_func=True, grad_norm_clip=10)
    return log


if __name__ == "__main__":
    torch.set_num_threads(4)
    R = load_reference()
    g1_vfe(R)
    g2_g3_memory_scatter(R)
    g4_backbone(R)
    g4_backbone_train(R)
    g5_head(R)
    g6_g7_coder(R)
    g8_assigner_losses(R)
    g9_onecycle(R)
    g10_train_memory(R)
    g11_preprocess(R)
    g12_kitti_eval(R)
    g13_voxel_index(R)
    g14_axis_aligned_iou(R)
    g15_post_processing(R)
    g16_train_branch_gradients(R)
    g17_train_loop_protocol(R)
    g18_assigner_edges(R)
    for f in sorted(os.listdir(OUT)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(OUT, f)) // 1024, "KB")
