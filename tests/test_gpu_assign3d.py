"""GPU: hvpr_assign_targets_ex_f32 — the target assigner with MATCH_HEIGHT (rotated 3-D IoU, k_assign3d) and NORM_BY_NUM_EXAMPLES.
The judge is the numpy host form of tests/assign3d_cases.py, which tests/test_assign3d_host.py pins to the reference's own assigner
through fixture G26: fed with the device's own pairwise table (hvpr_boxes_pairwise_f32 mode 2) the labels must be EXACTLY equal on
every anchor — the kernel's rejects, its compaction and its keyed maxima may not change a bit of the table — and against G26
itself labels and weights exact, targets 1e-5.  Every direct call runs twice on fresh buffers and must give the same bytes."""
import numpy as np
import pytest
import torch

import assign3d_cases as A3
import train_fixture_cases as C
from hvpr_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, INVALID_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # include/hvpr_amd.h hvpr_status
CAR = (3.9, 1.6, 1.56)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pairwise_iou3d(a, b):
    """The table the matcher is defined on, read back from the device."""
    if b.shape[0] == 0:
        return np.zeros((a.shape[0], 0), np.float32)
    return kernels.boxes_pairwise(_dev(a.astype(np.float32)), _dev(b.astype(np.float32)), 2).cpu().numpy()


def grid_anchors(nx=20, ny=24, spacing=0.32, size=CAR, z=-1.0, rots=(0.0, 1.57)):
    """(ny * nx * len(rots), 7) in the head's order (y, x, rotation)."""
    ys, xs = np.meshgrid(np.arange(ny) * spacing + spacing / 2, np.arange(nx) * spacing + spacing / 2, indexing="ij")
    a = np.zeros((ny, nx, len(rots), 7), np.float32)
    a[..., 0], a[..., 1], a[..., 2] = xs[..., None], ys[..., None], z
    a[..., 3:6] = size
    a[..., 6] = np.array(rots, np.float32)
    return a.reshape(-1, 7)


def random_gt(n, seed, rows=None, x=(0.5, 5.9), y=(0.5, 7.2)):
    """n cars over the 20 x 24 grid, the first half near an axis (IoU above the matched threshold exists), the rest at any heading."""
    r = np.random.default_rng(seed)
    g = np.zeros((rows or n, 8), np.float32)
    g[:n, 0], g[:n, 1], g[:n, 2] = r.uniform(*x, n), r.uniform(*y, n), r.uniform(-1.1, -0.9, n)
    g[:n, 3:6] = np.array(CAR) * r.uniform(0.9, 1.1, (n, 3))
    g[:n, 6] = np.where(np.arange(n) < (n + 1) // 2, r.choice([0, 1.57, -1.57, 3.1], n) + r.uniform(-0.12, 0.12, n), r.uniform(-np.pi, np.pi, n))
    g[:n, 7] = 1
    return g


def run_sets(sets, gt, n_classes, match_height, norm, entry="ex"):
    """Every anchor set of `sets` written into one head order by direct calls; twice, on fresh sentinel-filled buffers, the same bytes.
    Returns labels (B, A), targets (B, A, 7), weights (B, A), pos_count (B,) as numpy."""
    L = kernels.lib()
    B, G = gt.shape[0], gt.shape[1]
    gt_t = _dev(gt.astype(np.float32)) if G else torch.zeros((B, 1, 8), device=DEV)
    stride = sum(s[1] for s in sets)
    A = sets[0][0].shape[0] // sets[0][1] * stride

    def once():
        lab = torch.full((B, A), 77, dtype=torch.int32, device=DEV)
        tgt, w = torch.full((B, A, 7), 77.0, device=DEV), torch.full((B, A), 77.0, device=DEV)
        pos = torch.zeros((B,), dtype=torch.int32, device=DEV)
        off = 0
        for anchors, per_loc, ci, matched, unmatched in sets:
            a_t = _dev(anchors)
            args = (a_t, a_t.shape[0], gt_t, B, G, ci, n_classes, float(matched), float(unmatched), per_loc, stride, off, A, lab, tgt, w, pos)
            if entry == "ex":
                need = int(L.hvpr_assign_targets_ex_workspace_bytes(B, G, a_t.shape[0], match_height))
                ws = torch.full((need,), 77, dtype=torch.uint8, device=DEV)
                kernels.call("hvpr_assign_targets_ex_f32", *args, match_height, norm, ws, need, kernels._stream())
            else:
                need = max(int(L.hvpr_assign_targets_workspace_bytes(B, G)), 256)
                ws = torch.full((need,), 77, dtype=torch.uint8, device=DEV)
                kernels.call("hvpr_assign_targets_f32", *args, ws, need, kernels._stream())
            off += per_loc
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (lab, tgt, w, pos)]
    first, second = once(), once()
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    return first


def check(got, want, where):
    """Labels and weights exact on every anchor, targets 1e-5, pos_count the number of positives."""
    n_bad = int((got[0] != want[0]).sum())
    assert n_bad == 0, f"{where}: {n_bad} of {want[0].size} labels differ, positives {int((got[0] > 0).sum())} against {int((want[0] > 0).sum())}"
    np.testing.assert_array_equal(got[2], want[2], err_msg=where)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-5, atol=1e-6, err_msg=where)
    assert not got[1][want[0] <= 0].any(), where
    np.testing.assert_array_equal(got[3], (want[0] > 0).sum(axis=1), err_msg=where)


# ------------------------------------------------------------------------------------------------ (i) the table
def test_labels_equal_the_host_form_over_the_devices_own_table():
    """960 car anchors (20 x 24 locations 0.32 m apart, rotations 0 and 1.57), six ground truths: exact on 100 % of the anchors.  The
    case has anchors in all three label bands at 0.6 / 0.45, and every workgroup clips more than one round of 64 pairs."""
    anchors, gt = grid_anchors(), random_gt(6, 2600)[None]
    sets = [(anchors, 2, 0, 0.6, 0.45)]
    want = A3.host_assign(sets, gt, 1, False, pairwise_iou3d)
    best = pairwise_iou3d(anchors, gt[0, :, :7]).max(axis=1)
    assert (best >= 0.6).sum() >= 6 and ((best >= 0.45) & (best < 0.6)).sum() >= 20 and (want[0] == 0).sum() >= 500
    assert (want[0] > 0).sum() >= 6 and (want[0] == -1).sum() >= 20
    assert A3.pairs_per_workgroup(anchors, gt[0], 0, 1).min() > 64
    check(run_sets(sets, gt, 1, 1, 0), want, "table identity")


# ------------------------------------------------------------------------------------------------ (ii) edges
@pytest.mark.parametrize("A", [255, 256, 257, 960])
def test_anchor_counts_around_a_workgroup_and_a_block(A):
    """The first A anchors of the grid, one per location: the last workgroup holds 63, 64, 1 and 64 anchors."""
    anchors, gt = grid_anchors()[:A], random_gt(6, 2601, y=(0.5, 2.5))[None]
    sets = [(anchors, 1, 0, 0.6, 0.45)]
    want = A3.host_assign(sets, gt, 1, False, pairwise_iou3d)
    assert (want[0] > 0).sum() >= 4
    check(run_sets(sets, gt, 1, 1, 0), want, f"A {A}")


@pytest.mark.parametrize("G,n_real", [(0, 0), (1, 1), (50, 20), (256, 256)])
def test_ground_truth_counts_up_to_the_limit(G, n_real):
    """No row at all, one, 20 in 50 padded rows, and kMaxGt = 256 real rows (every LDS slot in use, thousands of pairs a workgroup)."""
    anchors = grid_anchors()
    gt = random_gt(n_real, 2602 + G, rows=max(G, 1))[None][:, :G]
    sets = [(anchors, 2, 0, 0.6, 0.45)]
    want = A3.host_assign(sets, gt, 1, True, pairwise_iou3d)
    got = run_sets(sets, gt, 1, 1, 1)
    check(got, want, f"G {G}")
    if n_real == 0:
        assert not got[0].any() and not got[1].any() and not got[2].any() and not got[3].any()
    else:
        assert (want[0] > 0).sum() >= n_real // 4 + 1


class _ExArgs:
    """Valid buffers and arguments of a direct hvpr_assign_targets_ex_f32 call (2 locations x 2 rotations, one class), outputs and
    workspace pre-filled with sentinels.  Keyword arguments replace single arguments; a pointer named in `null` goes as NULL."""

    def __init__(self, n_gt=4, null=(), **over):
        self.anchors = torch.tensor([[1.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0], [1.0, 0.0, -1.0, 3.9, 1.6, 1.56, 1.57],
                                     [3.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0], [3.0, 0.0, -1.0, 3.9, 1.6, 1.56, 1.57]], device=DEV)
        self.gt = torch.zeros(1, max(n_gt, 1), 8, device=DEV)
        self.gt[0, 0] = torch.tensor([1.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0, 1.0])
        self.labels = torch.full((1, 4), 77, dtype=torch.int32, device=DEV)
        self.targets = torch.full((1, 4, 7), 77.0, device=DEV)
        self.weights = torch.full((1, 4), 77.0, device=DEV)
        self.pos = torch.full((1,), 77, dtype=torch.int32, device=DEV)
        self.ws = torch.full((4096,), 77, dtype=torch.uint8, device=DEV)
        self.null = set(null)
        self.v = dict(n_anchors=4, batch=1, n_gt=n_gt, class_index=0, n_classes=1, matched=0.6, unmatched=0.45, rots=2, loc_stride=2,
                      loc_offset=0, anchors_total=4, match_height=1, norm=1, ws_bytes=self.ws.numel())
        self.v.update(over)

    def call(self):
        v = self.v
        p = lambda name: None if name in self.null else getattr(self, name).data_ptr()
        rc = kernels.lib().hvpr_assign_targets_ex_f32(
            p("anchors"), v["n_anchors"], p("gt"), v["batch"], v["n_gt"], v["class_index"], v["n_classes"], v["matched"], v["unmatched"],
            v["rots"], v["loc_stride"], v["loc_offset"], v["anchors_total"], p("labels"), p("targets"), p("weights"), p("pos"),
            v["match_height"], v["norm"], p("ws"), v["ws_bytes"], kernels._stream())
        torch.cuda.synchronize()
        return rc

    def assert_untouched(self):
        assert bool((self.labels == 77).all()) and bool((self.targets == 77).all()) and bool((self.weights == 77).all())
        assert bool((self.pos == 77).all()) and bool((self.ws == 77).all())


@pytest.mark.parametrize("match_height,norm", [(1, 0), (0, 1), (1, 1), (0, 0)])
def test_ex_entry_point_refusals_leave_the_outputs_untouched(match_height, norm):
    """257 ground truths, NULL pointers, negative sizes, an inconsistent head order and a short workspace: the status comes from the
    host checks above the first launch and nothing is written.  The same arguments without the fault run and label the anchor that
    IS the ground truth."""
    need = int(kernels.lib().hvpr_assign_targets_ex_workspace_bytes(1, 4, 4, match_height))
    assert need == 768
    flags = dict(match_height=match_height, norm=norm)
    cases = [(dict(n_gt=257), UNSUPPORTED), (dict(n_gt=-1), INVALID_ARG), (dict(n_anchors=-4), INVALID_ARG), (dict(batch=0), INVALID_ARG),
             (dict(rots=3, loc_stride=3), INVALID_ARG), (dict(class_index=1), INVALID_ARG), (dict(loc_stride=3, loc_offset=2, anchors_total=6), INVALID_ARG)]
    cases += [(dict(null=(name,)), INVALID_ARG) for name in ("anchors", "gt", "labels", "targets", "weights", "pos", "ws")]
    if match_height or norm:
        cases.append((dict(ws_bytes=need - 1), WORKSPACE))
    else:
        cases.append((dict(ws_bytes=int(kernels.lib().hvpr_assign_targets_workspace_bytes(1, 4)) - 1), WORKSPACE))
    for over, status in cases:
        a = _ExArgs(**{**flags, **over})
        assert a.call() == status, over
        a.assert_untouched()
    a = _ExArgs(ws_bytes=need, **flags)
    a.pos.zero_()
    assert a.call() == OK
    assert a.labels.tolist() == [[1, 0, 0, 0]] and a.pos.tolist() == [1]
    assert a.weights.tolist() == [[np.float32(1) / np.float32(4) if norm else 1.0, 0.0, 0.0, 0.0]]


def _g26_head(z, which, match_height, norm):
    head = C._g18_head(z, which, DEV)
    head.model_cfg.TARGET_ASSIGNER_CONFIG.MATCH_HEIGHT = bool(match_height)
    head.model_cfg.TARGET_ASSIGNER_CONFIG.NORM_BY_NUM_EXAMPLES = bool(norm)
    return head


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("which", ["car", "3c"])
def test_g26_frames_alone_and_in_batches_through_the_head(golden_dir, which):
    """The product's AnchorHeadSingle.assign_targets with MATCH_HEIGHT True against the reference's own outputs (fixture G26): G18's
    edge frames plus a ground truth identical to an anchor, one out of every anchor's reach, one over anchors in BEV but disjoint
    in z, a zero box in row 0, rows of a foreign class and of class 0, headings on +-pi/4, pi/2 and general, a frame that leaves a
    workgroup a single pair to clip and one with ten ground truths on one spot; for "3c" three anchor sets written into one head
    order.  Every frame alone (batch 1), NORM_BY_NUM_EXAMPLES off and on; then all frames as one batch and three of them as a
    batch of 3, bit for bit what the frames alone gave."""
    z = A3.load_g26(golden_dir)
    cases = [str(c) for c in z[which + ".cases"]]
    heads = {norm: _g26_head(z, which, True, norm) for norm in (False, True)}
    alone = {}
    for name in cases:
        gt = z[f"{which}.{name}.gt"]
        for norm in (False, True):
            t = heads[norm].assign_targets(_dev(gt)[None])
            got = tuple(_np(t[k][0]) for k in ("box_cls_labels", "box_reg_targets", "reg_weights"))
            A3.check_against_g26(z, which, name, norm, got, tag="gpu ")
            assert int(t["positives_per_frame"][0]) == int((got[0] > 0).sum())
            alone[name, norm] = got
        for k in (0, 1):                                       # labels and targets do not depend on NORM_BY_NUM_EXAMPLES: the same bits
            assert alone[name, False][k].tobytes() == alone[name, True][k].tobytes(), (name, k)
    batch = np.zeros((len(cases), int(z["pad_rows"]), 8), np.float32)
    for i, name in enumerate(cases):
        gt = z[f"{which}.{name}.gt"]
        batch[i, :len(gt)] = gt
    three = [cases.index(n) for n in ("stacked10", "only_padding", "random50")]
    for norm in (False, True):
        for rows in (list(range(len(cases))), three):
            whole = heads[norm].assign_targets(_dev(batch[rows]))
            for j, i in enumerate(rows):
                for k, key in enumerate(("box_cls_labels", "box_reg_targets", "reg_weights")):
                    assert _np(whole[key][j]).tobytes() == alone[cases[i], norm][k].tobytes(), (which, cases[i], key, norm)


def test_z_disjoint_ground_truth_forces_a_match_only_without_the_flag(golden_dir):
    z = A3.load_g26(golden_dir)
    gt = _dev(z["car.z_disjoint_only.gt"])[None]
    on, off = _g26_head(z, "car", True, False).assign_targets(gt), _g26_head(z, "car", False, False).assign_targets(gt)
    assert int(on["positives_per_frame"][0]) == 0 and not bool((on["box_cls_labels"] != 0).any())
    assert int(off["positives_per_frame"][0]) >= 1


# ------------------------------------------------------------------------------------------------ (iii) NORM_BY_NUM_EXAMPLES
@pytest.mark.parametrize("match_height", [1, 0])
def test_norm_by_num_examples_weights_per_frame_and_set(match_height):
    """Two anchor sets in one head order, three frames (20 rows, 3 rows, none): weights are float32(1) / float32(max(n, 1)) exactly, n
    counted per frame and set; labels, targets and pos_count the bits of the flag-off run; the empty frame has all-zero weights."""
    cars = grid_anchors()
    small = grid_anchors(size=(1.76, 0.6, 1.73), z=-0.6)
    sets = [(cars, 2, 0, 0.6, 0.45), (small, 2, 1, 0.5, 0.35)]
    gt = np.zeros((3, 24, 8), np.float32)
    gt[0, :20] = random_gt(20, 2610)
    gt[0, 10:20, 3:6] = np.array([1.76, 0.6, 1.73], np.float32)
    gt[0, 10:20, 7] = 2
    gt[1, :3] = random_gt(3, 2611)
    plain, normed = run_sets(sets, gt, 2, match_height, 0), run_sets(sets, gt, 2, match_height, 1)
    for k in (0, 1, 3):
        assert plain[k].tobytes() == normed[k].tobytes(), k
    lab = normed[0].reshape(3, -1, 2, 2)                       # (frame, location, set, rotation)
    w = normed[2].reshape(3, -1, 2, 2)
    for b in range(3):
        for s in range(2):
            n = max(int((lab[b, :, s] >= 0).sum()), 1)
            np.testing.assert_array_equal(w[b, :, s], np.where(lab[b, :, s] > 0, np.float32(1) / np.float32(n), np.float32(0)))
    assert (lab[0, :, 0] > 0).any() and (lab[0, :, 1] > 0).any() and (lab[1, :, 0] > 0).any() and (lab[0] == -1).any()
    assert not normed[2][2].any() and not normed[0][2].any()
    iou = pairwise_iou3d if match_height else (lambda a, b: _nearest(a, b))
    check(normed, A3.host_assign(sets, gt, 2, True, iou), f"norm, match_height {match_height}")


def _nearest(a, b):
    import torch_forms
    return torch_forms.boxes3d_nearest_bev_iou(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b))).numpy()


# ------------------------------------------------------------------------------------------------ (iv) both flags 0
@pytest.mark.parametrize("which", ["car", "3c"])
def test_both_flags_off_is_the_old_entry_point_bit_for_bit_on_g18(golden_dir, which):
    z = C._load(golden_dir, "g18_assigner_edges.npz")
    sets, names = A3.g26_anchor_sets(z, which)
    cases = [str(c) for c in z[which + ".cases"]]
    batch = np.zeros((len(cases), int(z["pad_rows"]), 8), np.float32)
    for i, name in enumerate(cases):
        gt = z[f"{which}.{name}.gt"]
        batch[i, :len(gt)] = gt
    old, new = run_sets(sets, batch, len(names), 0, 0, entry="old"), run_sets(sets, batch, len(names), 0, 0, entry="ex")
    for a, b in zip(old, new):
        assert a.tobytes() == b.tobytes()
    assert (old[0] > 0).sum() > 100
    for i, name in enumerate(cases):                           # ... and G18 itself: the reference's labels
        np.testing.assert_array_equal(new[0][i], z[f"{which}.{name}.labels"].astype(np.int32), err_msg=name)


# ------------------------------------------------------------------------------------------------ (v) one training epoch of three steps
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import train_driver_cases as D
    return D.write_tree_with_infos(tmp_path_factory.mktemp("kitti"))


def test_training_with_match_height_counts_the_host_forms_positives_and_adds_no_sync(tree):
    """The tiny KITTI tree of the driver tests, `--set MODEL.DENSE_HEAD.TARGET_ASSIGNER_CONFIG.MATCH_HEIGHT True`: finite losses,
    positives_per_frame of the last step equal to the host form's count on that batch, and under torch's sync debug mode (counted as
    tests/test_gpu_optim.py counts) no more synchronising calls in an epoch than with the flag off."""
    import train_driver_cases as D
    from hvpr_amd import anchor_head, config, optim, train_loop
    from hvpr_amd.detector import build_network
    from hvpr_amd.epoch_loader import build_dataloader
    counts, seen = {}, {}
    for name, set_cfgs in (("off", None), ("on", ["MODEL.DENSE_HEAD.TARGET_ASSIGNER_CONFIG.MATCH_HEIGHT", "True"])):
        cfg = D.model_cfg()
        if set_cfgs:
            config.cfg_from_list(list(set_cfgs), cfg)
        assert cfg.MODEL.DENSE_HEAD.TARGET_ASSIGNER_CONFIG.MATCH_HEIGHT is (name == "on")
        ds, loader, sampler = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 2, root_path=tree, training=True, seed=0, prefetch=False)
        torch.manual_seed(0)
        np.random.seed(0)
        model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda()
        opt = optim.build_optimizer(model, cfg.OPTIMIZATION)
        sched, _ = optim.build_scheduler(opt, len(loader), 4, -1, cfg.OPTIMIZATION)
        inner = optim.model_fn_decorator()
        batches, losses = [], []

        def fn(model, batch):
            out = inner(model, batch)
            batches.append(batch)
            losses.append(out[0].detach())
            return out
        it, _ = train_loop.train_one_epoch(model, opt, loader, fn, sched, 0, cfg.OPTIMIZATION)        # lazy initialisation
        torch.cuda.synchronize()
        sampler.set_epoch(1)
        (it, _), counts[name] = D.sync_warnings(lambda: train_loop.train_one_epoch(model, opt, loader, fn, sched, it, cfg.OPTIMIZATION))
        torch.cuda.synchronize()
        assert it == 6 and all(bool(torch.isfinite(x)) for x in losses)
        head = [m for m in model.modules() if isinstance(m, anchor_head.AnchorHeadSingle)][0]
        assert head.target_assigner.match_height is (name == "on")
        seen[name] = (head, batches[-1]["gt_boxes"].detach().cpu().numpy(), _np(head.forward_ret_dict["positives_per_frame"]),
                      _np(head.forward_ret_dict["box_cls_labels"]))
    assert counts["on"] <= counts["off"], counts
    head, gt, pos, labels = seen["on"]
    sets = [(a.reshape(-1, 7).cpu().numpy().astype(np.float32), int(a.shape[3] * a.shape[4]), k, head.target_assigner.matched[n],
             head.target_assigner.unmatched[n]) for k, (a, n) in enumerate(zip(head.anchors, head.target_assigner.anchor_class_names))]
    want = A3.host_assign(sets, gt, len(head.class_names), False, pairwise_iou3d)
    assert (want[0] > 0).sum() >= 1
    np.testing.assert_array_equal(pos, (want[0] > 0).sum(axis=1))
    np.testing.assert_array_equal(labels, want[0])
