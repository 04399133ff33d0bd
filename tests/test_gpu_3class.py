"""GPU: BASELINE.json configs[3] — the 3-class model (Car / Pedestrian / Cyclist, 6 anchors per location, SURVEY.md §8d
config 4): eval forward of a batch of two against the oracle, and training steps with multi-class target assignment."""
import numpy as np
import pytest
import torch

from hvpr_amd import detector, optim, synthetic, synthetic_weights
from hvpr_amd.config import hvpr_3class_cfg
from oracle import hvpr_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(got, ref, what, rtol=1e-3):
    """north_star's 1e-3 relative, ELEMENT-wise, the absolute term tied to the tensor's own rms (as tests/test_gpu_e2e._close)."""
    rms = float(np.sqrt(np.mean(np.square(ref, dtype=np.float64))))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=rtol * max(rms, 1e-30), err_msg=what)


def _batch(frames):
    pts = np.concatenate([np.concatenate([np.full((len(f), 1), b, np.float32), f], 1) for b, f in enumerate(frames)])
    return {"points": torch.from_numpy(pts).to(DEV), "batch_size": len(frames)}


def test_three_class_forward_matches_oracle():
    cfg = hvpr_3class_cfg()
    model = detector.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), detector.SyntheticDataset(cfg))
    params = synthetic_weights.load_synthetic(model, seed=5, cls_bias=-2.0)
    # spread the class logits so that all three labels occur (the synthetic head has one shared bias)
    with torch.no_grad():
        model.dense_head.conv_cls.bias += torch.tensor([0.0, -0.2, 0.1] * 6)
    params["dense_head.conv_cls.bias"] = model.dense_head.conv_cls.bias.detach().numpy().copy()
    model = model.to(DEV).eval()
    assert model.dense_head.num_anchors_per_location == 6 and model.dense_head.num_class == 3
    frames = [synthetic.hvpr_frame(50), synthetic.hvpr_frame(51)[:12000]]
    with torch.no_grad():
        preds, _, bd = model(_batch(frames))
    ref_preds, inter = O.forward_frames(frames, params, O.cfg_from_model_cfg(cfg))
    assert bd["batch_cls_preds"].shape == (2, 248 * 296 * 6, 3)
    _close(bd["spatial_features_2d"].cpu().numpy(), inter["spatial_features_2d"].numpy(), "spatial_features_2d")
    _close(bd["batch_cls_preds"].cpu().numpy(), inter["batch_cls_preds"].numpy(), "batch_cls_preds")
    gb, rb = bd["batch_box_preds"].cpu().numpy(), inter["batch_box_preds"].numpy()
    _close(gb[..., :6], rb[..., :6], "batch_box_preds[..., :6]")
    scores = bd["batch_max_scores"].cpu().numpy()
    labels_seen = set()
    for b in range(2):
        # survivors bit-exact when the oracle's NMS is fed the GPU's own scores and boxes; labels = argmax class + 1
        ref = O.class_agnostic_nms(scores[b], gb[b], 0.1, 0.1, 4096, 500)
        np.testing.assert_array_equal(preds[b]["selected"].cpu().numpy(), ref[0])
        # label = argmax over the class SIGMOIDS, first maximum on ties (detector3d_template.py:206-207): where two class
        # logits round to the same fp32 sigmoid the choice may differ from an argmax over the logits
        sig = torch.sigmoid(bd["batch_cls_preds"][b]).cpu().numpy()[ref[0]]
        got_labels = preds[b]["pred_labels"].cpu().numpy()
        picked = sig[np.arange(len(got_labels)), got_labels - 1]
        assert np.all(sig.max(axis=-1) - picked <= 2e-7), float((sig.max(axis=-1) - picked).max())
        labels_seen |= set(got_labels.tolist())
        a, o = set(ref[0].tolist()), set(ref_preds[b]["selected"].tolist())
        assert len(a & o) >= 0.9 * max(len(a), len(o), 1)
    assert labels_seen == {1, 2, 3}


def test_three_class_training_steps():
    cfg = hvpr_3class_cfg()
    model = detector.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), detector.SyntheticDataset(cfg, training=True))
    synthetic_weights.load_synthetic(model, seed=6, cls_bias=-4.595)
    model = model.to(DEV)
    opt = optim.build_optimizer(model, cfg.OPTIMIZATION)
    sched, _ = optim.build_scheduler(opt, total_iters_each_epoch=10, total_epochs=1, last_epoch=-1, optim_cfg=cfg.OPTIMIZATION)
    rng = np.random.default_rng(1)
    frames = [synthetic.hvpr_frame(60 + b, shuffle=True) for b in range(2)]
    bd = _batch(frames)
    gt = np.zeros((2, 9, 8), np.float32)
    sizes = {1: [3.9, 1.6, 1.56], 2: [0.8, 0.6, 1.73], 3: [1.76, 0.6, 1.73]}
    for b in range(2):
        for k in range(9 - b):                                     # ragged: trailing zero rows are padding
            c = 1 + k % 3
            gt[b, k] = [rng.uniform(5, 42), rng.uniform(-15, 15), rng.uniform(-1.2, -0.8), *sizes[c], rng.uniform(-3, 3), c]
    bd["gt_boxes"] = torch.from_numpy(gt).to(DEV)
    losses = []
    for it in range(3):
        loss, tb = optim.train_step(model, opt, sched, dict(bd), it, cfg.OPTIMIZATION.GRAD_NORM_CLIP)
        losses.append(float(loss))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    # every class got positive anchors of its own anchor block
    labels = model.dense_head.forward_ret_dict["box_cls_labels"]
    for c in (1, 2, 3):
        assert int((labels == c).sum()) > 0, c


def test_config4_three_class_train_step_batch8():
    """BASELINE.json configs[3] at ITS size, one GPU's share: hvpr 3-class, 8 frames of 16384 points per step (the 8 x MI355X job is
    eight of these under DDP).  Finite loss, every trainable parameter receives a finite gradient, the step changes the weights, a
    second whole step runs, every class gets positive anchors, peak memory recorded and bounded."""
    cfg = hvpr_3class_cfg()
    model = detector.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), detector.SyntheticDataset(cfg, training=True))
    synthetic_weights.load_synthetic(model, seed=8, cls_bias=-4.595)
    model = model.to(DEV).train()
    opt = optim.build_optimizer(model, cfg.OPTIMIZATION)
    sched, _ = optim.build_scheduler(opt, total_iters_each_epoch=10, total_epochs=1, last_epoch=-1, optim_cfg=cfg.OPTIMIZATION)
    rng = np.random.default_rng(8)
    B = 8
    bd = _batch([synthetic.hvpr_frame(300 + b, shuffle=True) for b in range(B)])
    assert bd["points"].shape == (B * 16384, 5)
    sizes = {1: [3.9, 1.6, 1.56], 2: [0.8, 0.6, 1.73], 3: [1.76, 0.6, 1.73]}
    gt = np.zeros((B, 9, 8), np.float32)
    for b in range(B):
        for k in range(9 - b % 3):
            c = 1 + (k + b) % 3
            gt[b, k] = [rng.uniform(5, 42), rng.uniform(-15, 15), rng.uniform(-1.2, -0.8), *sizes[c], rng.uniform(-3, 3), c]
    bd["gt_boxes"] = torch.from_numpy(gt).to(DEV)
    torch.cuda.reset_peak_memory_stats()
    sched.step(0)
    opt.zero_grad()
    ret, tb, _ = model(dict(bd))
    loss = ret["loss"].mean()
    assert torch.isfinite(loss)
    loss.backward()
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    assert not [k for k, p in named if p.grad is None]
    assert not [k for k, p in named if not torch.isfinite(p.grad).all()]
    nonzero = [k for k, p in named if float(p.grad.abs().max()) > 0]
    assert len(nonzero) >= 0.95 * len(named)
    labels = model.dense_head.forward_ret_dict["box_cls_labels"]
    assert labels.shape == (B, 248 * 296 * 6)
    for c in (1, 2, 3):
        assert int((labels == c).sum()) > 0, c
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    opt.clip_grad_norm(cfg.OPTIMIZATION.GRAD_NORM_CLIP)
    opt.step()
    model.update_global_step()
    assert all(not torch.equal(v, before[k]) for k, v in model.named_parameters() if k in nonzero[:50])
    loss2, _ = optim.train_step(model, opt, sched, dict(bd), 1, cfg.OPTIMIZATION.GRAD_NORM_CLIP)
    assert np.isfinite(float(loss2))
    peak = torch.cuda.max_memory_allocated() / 2**30
    print(f"config 4 (3-class, batch 8): loss {float(loss.detach()):.4f} -> {float(loss2):.4f}, peak memory {peak:.1f} GiB")
    assert peak < 150.0
