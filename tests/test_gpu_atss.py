"""GPU: hvpr_assign_targets_atss_f32 — the ATSS target assigner (TARGET_ASSIGNER_CONFIG.NAME: ATSS).  The judge is the numpy host
form of tests/atss_cases.py, which tests/test_atss_host.py pins to the reference's own ATSSTargetAssigner through fixture G27: fed
with the device's own pairwise table (hvpr_boxes_pairwise_f32 mode 1 / 2) labels and weights must be EXACTLY equal on every anchor
and targets within 1e-5 — the selection of the nearest, the statistics, the keyed maxima and the sweep's rejects may not change an
outcome.  The host form's margins (i) k-th against (k+1)-th distance and (iii) the inside test are asserted >= 1e-4 first, so an
input whose outcome hangs on rounding fails loudly instead of being skipped; exact ties are decided by the anchor index here as
there.  Every direct call runs twice on fresh sentinel-filled buffers and must give the same bytes."""
import numpy as np
import pytest
import torch

import assign3d_cases as A3
import atss_cases as AT
import train_fixture_cases as C
from hvpr_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, INVALID_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # include/hvpr_amd.h hvpr_status
CAR = (3.9, 1.6, 1.56)
KEYS = ("box_cls_labels", "box_reg_targets", "reg_weights")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def pairwise(mh):
    """The table the matcher is defined on, read back from the device: mode 1 (rotated BEV IoU) or 2 (rotated 3-D IoU)."""
    def iou(a, b):
        if b.shape[0] == 0:
            return np.zeros((a.shape[0], 0), np.float32)
        return kernels.boxes_pairwise(_dev(a.astype(np.float32)), _dev(b.astype(np.float32)), 2 if mh else 1).cpu().numpy()
    return iou


@pytest.fixture(scope="module")
def g27(golden_dir):
    return AT.load_g27(golden_dir)


@pytest.fixture(scope="module")
def grid(g27):
    """G18's car set: 40 x 32 locations, rotations 0 and 1.57 — 2560 anchors in the head's order (y, x, rotation)."""
    return AT.g27_anchor_sets(g27, "car")[0][0][0]


def random_gt(n, seed, rows=None, x=(0.4, 6.0), y=(-2.2, 2.2)):
    """n cars over G18's grid, half of them near an axis."""
    r = np.random.default_rng(seed)
    g = np.zeros((rows or n, 8), np.float32)
    g[:n, 0], g[:n, 1], g[:n, 2] = r.uniform(*x, n), r.uniform(*y, n), r.uniform(-1.1, -0.9, n)
    g[:n, 3:6] = np.array(CAR) * r.uniform(0.9, 1.1, (n, 3))
    g[:n, 6] = np.where(np.arange(n) < (n + 1) // 2, r.choice([0, 1.57, -1.57, 3.1], n) + r.uniform(-0.12, 0.12, n), r.uniform(-np.pi, np.pi, n))
    g[:n, 7] = 1
    return g


def run_sets(sets, gt, n_classes, topk, mh):
    """Every anchor set of `sets` written into one head order by direct calls; twice, on fresh sentinel-filled buffers and workspaces,
    the same bytes.  Returns labels (B, A), targets (B, A, 7), weights (B, A), pos_count (B,) as numpy."""
    L = kernels.lib()
    B, G = gt.shape[0], gt.shape[1]
    gt_t = _dev(gt.astype(np.float32)) if G else torch.zeros((B, 1, 8), device=DEV)
    stride = sum(p for _, p in sets)
    A = sets[0][0].shape[0] // sets[0][1] * stride

    def once(fill):
        lab = torch.full((B, A), 77, dtype=torch.int32, device=DEV)
        tgt, w = torch.full((B, A, 7), 77.0, device=DEV), torch.full((B, A), 77.0, device=DEV)
        pos = torch.zeros((B,), dtype=torch.int32, device=DEV)
        off = 0
        for anchors, per_loc in sets:
            a_t = _dev(anchors)
            need = int(L.hvpr_assign_targets_atss_workspace_bytes(B, G, a_t.shape[0], topk))
            assert need > 0
            ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
            kernels.call("hvpr_assign_targets_atss_f32", a_t, a_t.shape[0], gt_t, B, G, n_classes, topk, mh, per_loc, stride, off, A, lab,
                         tgt, w, pos, ws, need, kernels._stream())
            off += per_loc
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (lab, tgt, w, pos)]
    first, second = once(77), once(255)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    return first


def check(got, want, where):
    """Labels and weights exact on every anchor, targets 1e-5, pos_count the number of positives."""
    for b in range(want[0].shape[0]):
        AT.check_equal([g[b] for g in got[:3]], [w[b] for w in want[:3]], f"{where} frame {b}")
    np.testing.assert_array_equal(got[3], (want[0] > 0).sum(axis=1), err_msg=where)


def judged(sets, gt, n_classes, topk, mh, where, bar=1e-4):
    """The host form over the device's own table, its margins (i) and (iii) asserted first, against the device."""
    want = AT.host_atss(sets, gt, n_classes, topk, pairwise(mh))
    mg = want[3]
    assert mg["nearest"] >= bar and mg["inside"] >= bar and mg["on_face"] == 0, (where, mg)
    got = run_sets(sets, gt, n_classes, topk, mh)
    check(got, want, where)
    return got, want


# ------------------------------------------------------------------------------------------------ (i) the grid
@pytest.mark.parametrize("mh", [0, 1])
@pytest.mark.parametrize("topk", [1, 2, 8, 9, 64])
def test_grid_equals_the_host_form_over_the_devices_own_table(grid, topk, mh):
    """2560 car anchors (two chunks of the nearest kernel, 40 workgroups of the sweep), eight ground truths: a frame alone, and a
    batch of three with an empty frame (zero rows only) between two full ones.  TOPK 1 gives forced matches only; odd TOPK cuts
    inside a rotation pair and is decided by the anchor index."""
    sets = [(grid, 2)]
    gt = np.zeros((3, 10, 8), np.float32)
    gt[0, :8], gt[2, :6] = random_gt(8, 2700), random_gt(6, 2701)
    got, want = judged(sets, gt, 1, topk, mh, f"grid topk {topk} mh {mh}")
    alone, _ = judged(sets, gt[:1], 1, topk, mh, f"grid alone topk {topk} mh {mh}")
    for k in range(4):
        assert alone[k][0].tobytes() == got[k][0].tobytes()
    assert not got[0][1].any() and not got[1][1].any() and not got[2][1].any() and got[3][1] == 0
    n0, n2 = int((want[0][0] > 0).sum()), int((want[0][2] > 0).sum())
    if topk == 1:
        assert 1 <= n0 <= 8 and 1 <= n2 <= 6
    else:
        assert n0 >= 8 and n2 >= 6                               # every ground truth keeps an anchor here: eight and six centres apart
    if topk % 2:
        assert want[3]["ties"] >= 14


# ------------------------------------------------------------------------------------------------ (ii) edges
@pytest.mark.parametrize("A", [255, 256, 257])
def test_anchor_counts_around_a_workgroup_and_a_block(grid, A):
    """The first A anchors of the grid, one per location in the head's order: the last workgroup of the sweep holds 63, 64 and 1
    anchors, the last block of the write kernel 255, 256 and 1."""
    gt = random_gt(5, 2710, x=(0.4, 6.0), y=(-2.5, -2.1))[None]
    _, want = judged([(grid[:A], 1)], gt, 1, 8, 1, f"A {A}")
    assert (want[0] > 0).sum() >= 5


def test_a_chunk_border_inside_a_rotation_pair(grid):
    """Anchors 1 .. 2559: the two rotations of a location are rows 2i - 1 and 2i, so rows 2047 | 2048 — the border of the nearest
    kernel's chunks — split a pair, right under a ground truth; TOPK 9 cuts a pair too."""
    anchors = grid[1:]
    gt = np.zeros((1, 2, 8), np.float32)
    gt[0, 0] = [anchors[2047, 0] + 0.03, anchors[2047, 1] - 0.02, -1.0, 3.8, 1.7, 1.5, 0.1, 1]
    gt[0, 1] = random_gt(1, 2711)[0]
    assert np.array_equal(anchors[2047, :2], anchors[2048, :2]) and anchors[2047, 6] != anchors[2048, 6]
    for topk in (8, 9):
        _, want = judged([(anchors, 1)], gt, 1, topk, 0, f"chunk border topk {topk}")
        keys, _ = AT.distance_keys(anchors, gt[0, 0])
        assert {2047, 2048} <= set(np.argsort(keys)[:topk].tolist())
        assert want[0][0, 2047] == 1 or want[0][0, 2048] == 1


def test_topk_equal_to_the_anchor_count(grid):
    anchors = grid[:64]
    gt = random_gt(3, 2712, x=(0.4, 5.0), y=(-2.6, -2.4))[None]
    want = AT.host_atss([(anchors, 2)], gt, 1, 64, pairwise(0))
    assert want[3]["nearest"] == AT.INF and want[3]["inside"] >= 1e-4
    check(run_sets([(anchors, 2)], gt, 1, 64, 0), want, "topk == n_anchors")
    assert (want[0] > 0).sum() >= 3


@pytest.mark.parametrize("G,n_real", [(0, 0), (1, 1), (50, 20), (256, 256)])
def test_ground_truth_counts_up_to_the_limit(grid, G, n_real):
    """No row at all, one, 20 in 50 padded rows, and 256 real rows (every LDS slot of the sweep in use)."""
    gt = random_gt(n_real, 2720 + G, rows=max(G, 1))[None][:, :G]
    got, want = judged([(grid, 2)], gt, 1, 8, 1, f"G {G}")
    if n_real == 0:
        assert not got[0].any() and not got[1].any() and not got[2].any() and not got[3].any()
    else:
        assert (want[0] > 0).sum() >= n_real // 4 + 1


def test_ten_ground_truths_on_one_spot(grid):
    """G26's stacked10: ten boxes on one centre, headings 0.05 apart, share their nearest anchors — one anchor is a positive
    candidate of many (the lowest row of the highest IoU takes it) and forced anchors are shared (the highest row takes them)."""
    gt = A3.extra_frames("car")["stacked10"][None]
    for mh in (0, 1):
        want = AT.host_atss([(grid, 2)], gt, 1, 8, pairwise(mh))
        check(run_sets([(grid, 2)], gt, 1, 8, mh), want, f"stacked10 mh {mh}")
        table = pairwise(mh)(grid, gt[0, :, :7])
        assert len(set(table.argmax(axis=0).tolist())) < 10                  # a forced anchor is shared
        assert (want[0] > 0).sum() >= 2


def test_a_workgroup_whose_ring_holds_a_single_pair(grid):
    """G26's corner_reach: past the grid's far corner, it reaches a handful of anchors and is alone in their workgroups."""
    gt = A3.extra_frames("car")["corner_reach"][None]
    assert (A3.pairs_per_workgroup(grid, gt[0], 0, 1) == 1).any()
    for mh in (0, 1):
        _, want = judged([(grid, 2)], gt, 1, 8, mh, f"corner_reach mh {mh}")
        assert (want[0] > 0).sum() >= 1


@pytest.mark.parametrize("mh", [0, 1])
def test_three_anchor_sets_land_in_the_heads_order(g27, mh):
    """G18's three-class head (car, pedestrian, cyclist sets, 6 anchors a location) on its 50 random ground truths of all classes:
    every ground truth is matched against every set, each set is written at its offset of the head's order."""
    sets, names = AT.g27_anchor_sets(g27, "3c")
    gt = np.zeros((2, 50, 8), np.float32)
    gt[0], gt[1, :7] = g27["3c.random50.gt"], g27["3c.random50.gt"][40:47]
    got, want = judged(sets, gt, 3, 8, mh, f"three sets mh {mh}")
    lab = want[0][0].reshape(-1, 3, 2)
    assert all((lab[:, s] > 0).sum() >= 10 for s in range(3)) and set(np.unique(lab)) == {0, 1, 2, 3}


def test_a_centre_exactly_on_a_face_is_inside_on_the_device(g27):
    """face6 of atss_cases: the closed inside test; against the host form over the device's table and the reference's labels."""
    for tag, nudge, labels in (("face6", False, [1, 1, 0, 0, 0, 0]), ("face6_nudged", True, [1, 0, 0, 0, 0, 0])):
        anchors, gt, topk = AT.face6_case(nudge)
        for mh in (0, 1):
            want = AT.host_atss([(anchors, 1)], gt[None], 1, topk, pairwise(mh))
            assert want[3]["on_face"] == (0 if nudge else 1) and want[3]["thresh"] >= 1e-3
            got = run_sets([(anchors, 1)], gt[None], 1, topk, mh)
            check(got, want, f"{tag} mh {mh}")
            assert got[0][0].tolist() == labels == g27[f"{tag}.mh{mh}.labels"].tolist()


# ------------------------------------------------------------------------------------------------ (iii) G27 through the head
def _atss_head(z, which, topk, mh):
    head = C._g18_head(z, which, DEV)
    t = head.model_cfg.TARGET_ASSIGNER_CONFIG
    t.NAME, t.TOPK, t.MATCH_HEIGHT = "ATSS", topk, bool(mh)
    return head


@pytest.mark.parametrize("which", ["car", "3c"])
def test_g27_frames_alone_and_in_batches_through_the_head(g27, which):
    """The product's AnchorHeadSingle.assign_targets with NAME: ATSS against the reference's own ATSSTargetAssigner (fixture G27),
    every pinned frame alone (batch 1); then all frames as one batch and three of them as a batch of 3, bit for bit what the frames
    alone gave — pinned or not.  For "3c" three anchor sets are written into one head order (the reference's rows, stored per
    set, are mapped by atss_cases.g27_head_order)."""
    sets, names = AT.g27_anchor_sets(g27, which)
    cases = [str(c) for c in g27[which + ".cases"]]
    batch = np.zeros((len(cases), int(g27["pad_rows"]), 8), np.float32)
    for i, name in enumerate(cases):
        gt = g27[f"{which}.{name}.gt"]
        batch[i, :len(gt)] = gt
    three = [cases.index(n) for n in ("stacked10", "only_padding", "random50")]
    for topk, mh in AT.g27_runs(g27, which):
        head = _atss_head(g27, which, topk, mh)
        alone, n_pinned = {}, 0
        for name in cases:
            gt, pinned, per_set = AT.g27_case(g27, which, topk, mh, name)
            t = head.assign_targets(_dev(gt)[None])
            got = tuple(_np(t[k][0]) for k in KEYS)
            assert t["box_cls_labels"].dtype == torch.int32 and int(t["positives_per_frame"][0]) == int((got[0] > 0).sum())
            assert pinned or name not in AT.atss_frames(which), (which, topk, mh, name)
            if pinned:
                n_pinned += 1
                AT.check_equal(got, AT.g27_head_order(sets, per_set), f"gpu {which} topk {topk} mh {mh} {name}")
            alone[name] = got
        assert n_pinned >= 8
        for rows in (list(range(len(cases))), three):
            whole = head.assign_targets(_dev(batch[rows]))
            for j, i in enumerate(rows):
                for k, key in enumerate(KEYS):
                    assert _np(whole[key][j]).tobytes() == alone[cases[i]][k].tobytes(), (which, topk, mh, cases[i], key)


# ------------------------------------------------------------------------------------------------ (iv) refusals
class _Args:
    """Valid buffers and arguments of a direct call (2 locations x 2 rotations, one class), outputs and workspace pre-filled with
    sentinels.  Keyword arguments replace single arguments; a pointer named in `null` goes as NULL."""

    def __init__(self, n_gt=4, null=(), **over):
        self.anchors = torch.tensor([[1.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0], [1.0, 0.0, -1.0, 3.9, 1.6, 1.56, 1.57],
                                     [3.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0], [3.0, 0.0, -1.0, 3.9, 1.6, 1.56, 1.57]], device=DEV)
        self.gt = torch.zeros(1, max(n_gt, 1), 8, device=DEV)
        self.gt[0, 0] = torch.tensor([1.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0, 1.0])
        self.labels = torch.full((1, 4), 77, dtype=torch.int32, device=DEV)
        self.targets = torch.full((1, 4, 7), 77.0, device=DEV)
        self.weights = torch.full((1, 4), 77.0, device=DEV)
        self.pos = torch.full((1,), 77, dtype=torch.int32, device=DEV)
        self.ws = torch.full((1 << 20,), 77, dtype=torch.uint8, device=DEV)
        self.null = set(null)
        self.v = dict(n_anchors=4, batch=1, n_gt=n_gt, n_classes=1, topk=2, mh=0, per_loc=2, loc_stride=2, loc_offset=0, anchors_total=4,
                      ws_bytes=self.ws.numel())
        self.v.update(over)

    def call(self):
        v = self.v
        p = lambda name: None if name in self.null else getattr(self, name).data_ptr()
        rc = kernels.lib().hvpr_assign_targets_atss_f32(
            p("anchors"), v["n_anchors"], p("gt"), v["batch"], v["n_gt"], v["n_classes"], v["topk"], v["mh"], v["per_loc"], v["loc_stride"],
            v["loc_offset"], v["anchors_total"], p("labels"), p("targets"), p("weights"), p("pos"), p("ws"), v["ws_bytes"], kernels._stream())
        torch.cuda.synchronize()
        return rc

    def assert_untouched(self):
        assert bool((self.labels == 77).all()) and bool((self.targets == 77).all()) and bool((self.weights == 77).all())
        assert bool((self.pos == 77).all()) and bool((self.ws == 77).all())


@pytest.mark.parametrize("mh", [0, 1])
def test_refusals_leave_the_outputs_untouched(mh):
    """NULL pointers, TOPK 0 / 65 / above the anchor count, a workspace one byte short, 257 rows, an inconsistent head order: the
    status comes from the host checks above the first launch and nothing is written.  The same arguments without the fault run."""
    need = int(kernels.lib().hvpr_assign_targets_atss_workspace_bytes(1, 4, 4, 2))
    assert 0 < need <= 4096
    cases = [(dict(topk=0), INVALID_ARG), (dict(topk=65), INVALID_ARG), (dict(topk=5), INVALID_ARG), (dict(n_gt=257), UNSUPPORTED),
             (dict(n_gt=-1), INVALID_ARG), (dict(n_anchors=-4), INVALID_ARG), (dict(batch=0), INVALID_ARG), (dict(n_classes=0), INVALID_ARG),
             (dict(per_loc=3, loc_stride=3), INVALID_ARG), (dict(loc_stride=3, loc_offset=2, anchors_total=6), INVALID_ARG),
             (dict(anchors_total=3), INVALID_ARG), (dict(ws_bytes=need - 1), WORKSPACE)]
    cases += [(dict(null=(name,)), INVALID_ARG) for name in ("anchors", "gt", "labels", "targets", "weights", "pos", "ws")]
    for over, status in cases:
        a = _Args(**{**dict(mh=mh), **over})
        assert a.call() == status, over
        a.assert_untouched()
    big = _Args(mh=mh, topk=65, n_anchors=4)                     # TOPK 65 with enough anchors is the limit, not the argument
    big.anchors = torch.zeros(66, 7, device=DEV)
    big.v.update(n_anchors=66, anchors_total=66)
    assert big.call() == UNSUPPORTED
    big.assert_untouched()
    a = _Args(ws_bytes=need, mh=mh)
    a.pos.zero_()
    assert a.call() == OK
    assert a.labels.tolist() == [[1, 0, 0, 0]] and a.pos.tolist() == [1] and a.weights.tolist() == [[1.0, 0.0, 0.0, 0.0]]
    assert bool((a.ws[need:] == 77).all())


# ------------------------------------------------------------------------------------------------ (v) capture, no host read
def test_captured_call_replayed_on_new_ground_truths_matches_the_eager_bytes(grid):
    L = kernels.lib()
    a_t = _dev(grid)
    B, G, A, topk = 2, 12, grid.shape[0], 9
    frames = [np.stack([random_gt(8, s, rows=G), random_gt(5, s + 50, rows=G)]) for s in (2730, 2731, 2732)]
    gt = _dev(frames[0])
    need = int(L.hvpr_assign_targets_atss_workspace_bytes(B, G, A, topk))
    lab = torch.empty((B, A), dtype=torch.int32, device=DEV)
    tgt, w = torch.empty((B, A, 7), device=DEV), torch.empty((B, A), device=DEV)
    pos = torch.empty((B,), dtype=torch.int32, device=DEV)
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)

    def step():
        pos.zero_()
        kernels.call("hvpr_assign_targets_atss_f32", a_t, A, gt, B, G, 1, topk, 1, 2, 2, 0, A, lab, tgt, w, pos, ws, need, kernels._stream())
    eager = []
    for f in frames:
        gt.copy_(_dev(f))
        step()
        torch.cuda.synchronize()
        eager.append([_np(t).tobytes() for t in (lab, tgt, w, pos)])
    assert eager[0] != eager[1] and eager[1] != eager[2]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        step()
    for f, want in zip(frames[::-1], eager[::-1]):
        gt.copy_(_dev(f))
        for t in (lab, tgt, w):
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        assert [_np(t).tobytes() for t in (lab, tgt, w, pos)] == want


def test_the_call_makes_no_host_read(g27):
    head = _atss_head(g27, "3c", 9, 1)
    gt = _dev(np.stack([g27["3c.random50.gt"], g27["3c.random50.gt"][::-1].copy()]))
    head.assign_targets(gt)                                       # the cached anchor sets
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = head.assign_targets(gt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(out["positives_per_frame"].sum()) >= 6


# ------------------------------------------------------------------------------------------------ (vi) dispatch, one training epoch
def test_the_head_dispatches_on_the_assigner_name(g27):
    from hvpr_amd import target_assigner
    gt = _dev(g27["car.random50.gt"])[None]
    head = _atss_head(g27, "car", 9, 0)
    out = head.assign_targets(gt)
    assert isinstance(head.target_assigner, target_assigner.ATSSTargetAssigner) and head.target_assigner.topk == 9
    assert int(out["positives_per_frame"][0]) >= 10 and int(out["box_cls_labels"].min()) == 0          # no -1 band
    plain = C._g18_head(g27, "car", DEV)
    ref = plain.assign_targets(gt)
    assert isinstance(plain.target_assigner, target_assigner.AxisAlignedTargetAssigner) and ref["box_cls_labels"].shape == out["box_cls_labels"].shape
    head = _atss_head(g27, "car", 9, 0)
    head.model_cfg.TARGET_ASSIGNER_CONFIG.pop("TOPK")
    with pytest.raises(KeyError, match="TOPK"):
        head.assign_targets(gt)
    head.model_cfg.TARGET_ASSIGNER_CONFIG.NAME = "Other"
    with pytest.raises(NotImplementedError):
        head.assign_targets(gt)


def test_no_ground_truth_rows_through_the_head_give_background(g27):
    """Deviation (d): a (B, 0, 8) tensor — no address to pass — gives all-background frames where the reference raises."""
    head = _atss_head(g27, "3c", 9, 1)
    out = head.assign_targets(torch.zeros((2, 0, 8), device=DEV))
    assert out["box_cls_labels"].shape == (2, 40 * 32 * 6) and out["box_reg_targets"].shape == (2, 40 * 32 * 6, 7)
    assert not bool(out["box_cls_labels"].any()) and not bool(out["box_reg_targets"].any()) and not bool(out["reg_weights"].any())
    assert out["positives_per_frame"].tolist() == [0, 0]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import train_driver_cases as D
    return D.write_tree_with_infos(tmp_path_factory.mktemp("kitti"))


def _atss_model_cfg():
    """train_driver_cases.model_cfg() on hvpr_car_atss.yaml: the shipped file, the tiny frames' augmentor and NUM_POINTS."""
    import train_driver_cases as D
    from hvpr_amd import config
    cfg, plain = config.hvpr_car_atss_cfg(), D.model_cfg()
    cfg.DATA_CONFIG = plain.DATA_CONFIG
    cfg.MODEL.POST_PROCESSING = plain.MODEL.POST_PROCESSING
    t = cfg.MODEL.DENSE_HEAD.TARGET_ASSIGNER_CONFIG
    assert t.NAME == "ATSS" and t.TOPK == 9
    t2 = dict(t)
    t2.pop("TOPK")
    assert {**t2, "NAME": "AxisAlignedTargetAssigner"} == dict(plain.MODEL.DENSE_HEAD.TARGET_ASSIGNER_CONFIG)
    return cfg


def test_training_with_the_atss_yaml_counts_the_host_forms_positives_and_adds_no_sync(tree):
    """One epoch of three steps on the tiny KITTI tree of the driver tests with hvpr_car_atss.yaml: finite losses, positives_per_frame
    and labels of the last step equal to the host form's on the full anchor set (146 816 anchors), and under torch's sync debug
    mode (counted as tests/test_gpu_optim.py counts) no more synchronising calls in an epoch than with the shipped config."""
    import train_driver_cases as D
    from hvpr_amd import anchor_head, optim, target_assigner, train_loop
    from hvpr_amd.detector import build_network
    from hvpr_amd.epoch_loader import build_dataloader
    counts, seen = {}, {}
    for name, cfg in (("shipped", D.model_cfg()), ("atss", _atss_model_cfg())):
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
        assert isinstance(head.target_assigner, target_assigner.ATSSTargetAssigner) is (name == "atss")
        seen[name] = (head, batches[-1]["gt_boxes"].detach().cpu().numpy(), _np(head.forward_ret_dict["positives_per_frame"]),
                      _np(head.forward_ret_dict["box_cls_labels"]))
    assert counts["atss"] <= counts["shipped"], counts
    head, gt, pos, labels = seen["atss"]
    sets = [(a.reshape(-1, 7).cpu().numpy().astype(np.float32), int(a.shape[3] * a.shape[4])) for a in head.anchors]
    want = AT.host_atss(sets, gt, len(head.class_names), 9, pairwise(0))
    assert (want[0] > 0).sum() >= 1 and want[0].shape[1] == 146816
    np.testing.assert_array_equal(pos, (want[0] > 0).sum(axis=1))
    np.testing.assert_array_equal(labels, want[0])
