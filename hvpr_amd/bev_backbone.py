"""2-D BEV backbone with the reference's plugin interface (pcdet/models/backbones_2d/base_bev_backbone.py,
spatial_attention.py): same registry key, ctor kwargs and state-dict names.  The eval forward runs every convolution
on the fp32 matrix cores through hvpr_conv2d_nhwc_f32 with BatchNorm / ReLU / gate / residual fused in the epilogue,
activations kept NHWC end to end, the gate computed ONCE per level (it depends only on the scale stream,
base_bev_backbone.py:289-293) and each deconv writing straight into its slice of the 384-channel concat.

The eval forward is a plan and two steps.  _build_plan folds and packs, for the selected conv_precision only, what every level
launches (_Level, in launch order); _trunk and _branch enqueue one level's layers through kernels.conv2d_nhwc, which picks the
kernel from the packed type; _Fork owns the HIP streams the branches run on.  forward() runs every level; forward_head() /
forward_tail() run the same steps as two halves on caller-owned boundary buffers (split_buffers), which the frame pipeline
overlaps between neighbouring frames."""
import collections
import contextlib
import os

import torch
import torch.nn as nn

from . import kernels
from .folding import FoldCached, bn_scale_shift


class ConvLayer(nn.Module):
    """spatial_attention.py:9-45 — conv (+bias) + BatchNorm2d, no activation here."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, use_norm=True, activation=False):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding)
        self.norm = nn.BatchNorm2d(out_channels, eps=1e-3, momentum=0.01) if use_norm else None
        self.relu = nn.ReLU() if activation else None


class SpatialAttention(nn.Module):
    """CBAM-style spatial gate — spatial_attention.py:51-63.  forward(x, w) = sigmoid(BN(conv(pool(w)))) * x."""

    def __init__(self):
        super().__init__()
        self.spatial = ConvLayer(2, 1, 3, stride=1, padding=1, use_norm=True, activation=False)

    def gate_params(self):
        s, t = bn_scale_shift(self.spatial.norm)
        return (self.spatial.conv.weight.detach().float().reshape(18).contiguous(), float(self.spatial.conv.bias.detach()),
                float(s), float(t))


def _conv_bn_relu(cin, cout, stride=1, zero_pad=False):
    if zero_pad:   # nn.ZeroPad2d(1) + conv(padding=0) — the form the reference uses for strided entries (:154-160)
        return [nn.ZeroPad2d(1), nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=0, bias=False),
                nn.BatchNorm2d(cout, eps=1e-3, momentum=0.01), nn.ReLU()]
    return [nn.Conv2d(cin, cout, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(cout, eps=1e-3, momentum=0.01), nn.ReLU()]


def _block(cin, cout, stride, layer_num):
    """One level's trunk: the strided entry convolution and layer_num more."""
    layers = _conv_bn_relu(cin, cout, stride, zero_pad=True)
    for _ in range(layer_num):
        layers += _conv_bn_relu(cout, cout)
    return nn.Sequential(*layers)


def _deblock(cin, cout, stride):
    """One level's upsampling into the concat: ConvTranspose2d with kernel == stride."""
    return nn.Sequential(nn.ConvTranspose2d(cin, cout, int(stride), stride=int(stride), bias=False),
                         nn.BatchNorm2d(cout, eps=1e-3, momentum=0.01), nn.ReLU())


# Workgroup tile of hvpr_conv2d_nhwc_f32 (0 = 128 px x 128 ch, 1 = 64 px x 64 ch, 2 = 128 px x 64 ch): 64 x 64 on every layer group (trunk,
# SFM, scale, deconv) and level.  Measured on MI355X at batch 1 inside the whole frame (bench.py; the streams of the backbone interact, so
# the per-layer micro-benchmarks tools/bench_conv.py / bench_conv1x1.py do not decide alone); the sweeps are in profiles/NOTES_r04.md.
# The k = s = 4 deconvolution of level 2 (K = 512, 2048 columns, 4.6 k pixels) is bound by what its tiles pull out of L2 and 128 x 64
# halves its weight traffic per FLOP (121 -> 111 us alone): that won 0.2 % in round 1's 3-stage pipeline, 64 x 64 wins 0.7 % in the
# 4-stage one.
_TILE_CFG = 1
# Pixel groups per workgroup of the Winograd kernel: 1 = 8 x 16 px x 64 channels on every level (16 x 16 px workgroups and 32-channel
# tiles were measured slower inside the frame pipeline, profiles/NOTES_r04.md).
_WINO_PX_GROUPS = 1

# What the eval forward launches for one level, in launch order: trunk (packed layers), then on the branch scale, the gate (parameters
# of kernels.spatial_gate), sfm_steps (one packed layer per SFM iteration) and deconv into out[..., coff:coff + up_filters[index]].
_Level = collections.namedtuple("_Level", "index trunk scale gate sfm_steps deconv coff")
_Plan = collections.namedtuple("_Plan", "levels planes")          # planes: bf16 planes per value of the trunk's activations, 0 = fp32


def _fold_pack(pack, conv, bn, **kw):
    """Fold the eval-mode BatchNorm `bn` into `conv`'s weights and pack them with kernels.pack_*."""
    scale, shift = bn_scale_shift(bn)
    return pack(conv.weight, scale, shift, **kw)


def _conv_f32(conv, bn, stride=1):
    # stride-1 3x3 layers: Winograd F(2x2,3x3) kernel unless HVPR_CONV_ALGO=direct (kernels.pack_conv_auto)
    return _fold_pack(kernels.pack_conv_auto, conv, bn, stride=stride, tile_cfg=_TILE_CFG, px_groups=_WINO_PX_GROUPS)


def _deconv_f32(de):
    return _fold_pack(kernels.pack_deconv, de[0], de[1], tile_cfg=_TILE_CFG)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()       # no copy when the scatter produced channels_last


class _Fork:
    """HIP streams and allocator lifetime of one eval-forward call.  The trunk (blocks of level i+1) does not depend on the attentive
    branch of level i (scale conv, gate, the weight-shared SFM steps and the deconv), and the branches depend on each other only
    through the scale stream y_i = scale_i(y_{i-1}).  The trunk runs on the caller's stream, every branch on sides[i] (waiting for its
    x_i and, by event, for y_{i-1}): at batch 1 the upper levels have fewer tiles than the chip has workgroup slots.  sides = []: the
    branches stay in line on the caller's stream."""

    __slots__ = ("main", "sides", "used", "held", "y_event", "y_side", "eager")

    def __init__(self, sides):
        self.main, self.sides, self.used = torch.cuda.current_stream(), sides, []
        # tensors another stream reads: referenced until the join, so that the allocator of the producing stream cannot hand their
        # memory out again while the other stream still reads them
        self.held = []
        self.y_event = self.y_side = None
        self.eager = not torch.cuda.is_current_stream_capturing()      # eager mode: record_stream keeps the caching allocator from recycling early

    def branch(self, i, x, out):
        """The stream context level i's branch is enqueued in."""
        if not self.sides:
            return contextlib.nullcontext()
        side = self.sides[i]
        self.used.append(side)
        side.wait_stream(self.main)                 # x_i (and, at level 0, the scale stream's input) are ready for the branch
        if self.y_event is not None and self.y_side is not side:
            side.wait_event(self.y_event)           # y_{i-1} from the previous branch's stream
        self.held.append(x)
        if self.eager:
            x.record_stream(side)
            out.record_stream(side)
        return torch.cuda.stream(side)

    def y_ready(self, i, y):
        """y_i is enqueued (call inside branch(i)): the next level's branch waits for this point, not for the whole branch."""
        if self.sides:
            self.y_side = self.sides[i]
            self.y_event = torch.cuda.Event()
            self.y_event.record(self.y_side)
            self.held.append(y)
            if self.eager:
                y.record_stream(self.y_side)
                if i + 1 < len(self.sides):
                    y.record_stream(self.sides[i + 1])

    def join(self):
        for side in dict.fromkeys(self.used):       # only the streams this call forked (the other half of a split forward may own the others)
            self.main.wait_stream(side)
        self.held.clear()


def _trunk(lv, x, out=None):
    """The level's trunk convolutions, the last one into `out` when given."""
    for pc in lv.trunk[:-1]:
        x = kernels.conv2d_nhwc(x, pc, use_table=True)
    return kernels.conv2d_nhwc(x, lv.trunk[-1], out=out, use_table=True)


def _branch(lv, x, y, out, fork, y_out=None):
    """The level's attentive branch on x = its trunk output and y = the scale stream: scale conv (into `y_out` when given), gate, SFM
    steps, deconv into the level's slice of `out`.  Returns the level's scale output, the next level's y."""
    with fork.branch(lv.index, x, out):
        y = kernels.conv2d_nhwc(y, lv.scale, out=y_out, use_table=True)
        fork.y_ready(lv.index, y)
        gate = kernels.spatial_gate(y, *lv.gate)
        for pc in lv.sfm_steps:
            x = kernels.conv2d_nhwc(x, pc, gate=gate, resid=x, use_table=True)
            fork.held.append(x)
        fork.held.append(gate)
        kernels.conv2d_nhwc(x, lv.deconv, out=out, out_coff=lv.coff, use_table=True)
    return y


class _BEVTrunk(FoldCached):
    """What both backbones' eval forwards share, over the subclass's blocks, deblocks, layer_strides, layer_nums, upsample_strides
    and up_filters: every level's packed trunk with its deblock and slice of the concat, and the concat canvas."""

    def _trunks(self, conv):
        """(level, packed trunk, deblock, channel offset in the concat) of every level; conv(conv, bn, stride=1) folds and packs."""
        coff = 0
        for i, blk in enumerate(self.blocks):
            trunk = [conv(blk[1], blk[2], stride=self.layer_strides[i])]
            trunk += [conv(blk[4 + 3 * k], blk[5 + 3 * k]) for k in range(self.layer_nums[i])]
            yield i, trunk, self.deblocks[i], coff
            coff += self.up_filters[i]

    def _canvas(self, x):
        """The concat for the NHWC input x, empty: level-0 resolution after its own stride, times its upsample stride."""
        B, H, W, _ = x.shape
        s0, us0 = self.layer_strides[0], int(self.upsample_strides[0])
        return torch.empty((B, ((H + 2 - 3) // s0 + 1) * us0, ((W + 2 - 3) // s0 + 1) * us0, self.num_bev_features),
                           dtype=torch.float32, device=x.device)


class BaseBEVBackbone_Scale(_BEVTrunk):
    """base_bev_backbone.py:116-315."""

    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        layer_nums, strides, filters = list(model_cfg.LAYER_NUMS), list(model_cfg.LAYER_STRIDES), list(model_cfg.NUM_FILTERS)
        assert len(layer_nums) == len(strides) == len(filters)
        self.sfm_layer_nums = list(model_cfg.SFM_LAYER_NUMS)
        up_strides, up_filters = list(model_cfg.UPSAMPLE_STRIDES), list(model_cfg.NUM_UPSAMPLE_FILTERS)
        assert len(up_strides) == len(up_filters) == len(layer_nums), "HIP path: one deblock per level"
        scale_filters = list(model_cfg.NUM_SCALE_FILTERS)
        assert len(scale_filters) == len(strides)
        cin = [input_channels] + filters[:-1]
        cin_s = [input_channels // 4] + scale_filters[:-1]
        self.layer_strides, self.layer_nums, self.upsample_strides = strides, layer_nums, up_strides
        self.sfmblocks_down, self.sfmblocks_up = nn.ModuleList(), nn.ModuleList()
        self.scale_layers, self.blocks, self.deblocks = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for i in range(len(layer_nums)):
            self.blocks.append(_block(cin[i], filters[i], strides[i], layer_nums[i]))
            self.sfmblocks_down.append(nn.Sequential(*_conv_bn_relu(filters[i], filters[i])))
            s = up_strides[i]
            assert s >= 1 and int(s) == s, "HIP path: integer upsample strides (ConvTranspose2d with kernel == stride)"
            self.deblocks.append(_deblock(filters[i], up_filters[i], s))
            self.scale_layers.append(nn.Sequential(*_conv_bn_relu(cin_s[i], scale_filters[i], strides[i], zero_pad=True)))
        self.up_filters = up_filters
        self.num_bev_features = sum(up_filters)
        self.attention = SpatialAttention()
        self._sides = None
        # HIP streams of the eval forward: "1" none, "2" trunk + one branch stream, "4" trunk + one stream per level's branch
        self.n_streams = int(os.environ.get("HVPR_BEV_STREAMS", "4"))
        # "fp32": exact fp32 matrix-core kernel (default, the parity reference).  "bf16x3" / "bf16x6": trunk and SFM 3x3
        # convolutions on the bf16 matrix cores with operands split into 2 / 3 bf16 planes (kernels.conv2d_nhwc_bf3):
        # ~5e-6 relative error per layer / the fp32 kernel's own ~1.5e-6 (fp32 emulation)
        self.conv_precision = os.environ.get("HVPR_CONV_PRECISION", model_cfg.get("CONV_PRECISION", "fp32"))
        assert self.conv_precision in self.PRECISIONS

    PRECISIONS = {"fp32": 0, "bf16x3": 2, "bf16x6": 3}      # name -> bf16 planes per value

    def set_conv_precision(self, precision):
        assert precision in self.PRECISIONS
        self.conv_precision = precision
        self._fold.invalidate()

    def _streams(self, device):
        """The stream of every level's attentive branch (_Fork): one each (n_streams == 4), one shared by all (2), [] = in line (1)."""
        n = len(self.blocks)
        if self.n_streams == 1:
            return []
        if self._sides is None or len(self._sides) != n or self._sides[0].device != device:
            own = [torch.cuda.Stream(device=device) for _ in range(n if self.n_streams >= 4 else 1)]
            self._sides = [own[i % len(own)] for i in range(n)]
        return self._sides

    def _build_plan(self):
        """Every level's trunk and deconvolution, plus its scale conv, gate and SFM steps; in split-bf16 planes when selected."""
        planes = self.PRECISIONS[self.conv_precision]

        def conv_bf3(conv, bn, stride=1):
            # tile_cfg 4: 64 px x 64 ch tiles, weights staged per kernel row (2-3 workgroups per CU)
            return _fold_pack(kernels.pack_conv_bf3, conv, bn, stride=stride, tile_cfg=4, planes=planes)

        conv = conv_bf3 if planes else _conv_f32         # trunk and SFM layers; the scale stream is always fp32
        gate = self.attention.gate_params()
        levels = []
        for i, trunk, de, coff in self._trunks(conv):
            sfm = conv(*self.sfmblocks_down[i][:2])
            scale = _conv_f32(*self.scale_layers[i][1:3], stride=self.layer_strides[i])
            # two planes: the deconvolution runs split as well; three planes: its six-product 1x1 is slower than the fp32 kernel
            if planes == 2 and de[0].weight.shape[0] % 64 == 0:
                deconv = _fold_pack(kernels.pack_deconv_bf3, de[0], de[1], planes=planes)
            else:
                deconv = _deconv_f32(de)
            sfm_steps = [sfm] * self.sfm_layer_nums[i]
            if planes and sfm_steps and isinstance(deconv, kernels.PackedConv):
                sfm_steps[-1] = sfm.fp32_output()          # the last step hands fp32 to the deconvolution only when that one runs on the fp32 kernel
            levels.append(_Level(i, trunk, scale, gate, sfm_steps, deconv, coff))
        return _Plan(levels, planes)

    def _forward_train(self, data_dict):
        """Training forward, base_bev_backbone.py:228-279: the memory-fed and the point-fed canvases go through the SAME
        weights (two streams, shared scale stream); BatchNorm uses batch statistics and every call of a shared BN layer
        updates its running statistics.

        One code path: the library's own kernels through hvpr_amd.conv_train — forward / data-gradient convolutions on
        hvpr_conv2d_wino_nhwc_f32 / hvpr_conv2d_nhwc_f32, weight gradients on hvpr_conv2d_wino_wgrad_nhwc_f32 /
        hvpr_conv2d_wgrad_nhwc_f32, train-mode BatchNorm + ReLU on the hvpr_bn_* kernels, NHWC activations end to end.  CPU
        tensors and unsupported channel counts raise (the torch form of this forward is test infrastructure:
        tests/torch_forms.py)."""
        if not data_dict["spatial_features"].is_cuda:
            raise RuntimeError("hvpr_amd: BaseBEVBackbone_Scale's training forward needs GPU tensors (the HIP path has no CPU fallback)")
        from . import conv_train as ct

        def nhwc(t):
            return t.permute(0, 2, 3, 1).contiguous()          # no copy for the channels_last canvases of the scatter

        def cbr(seq, t, gate=None, resid=None):
            """Sequential of [ZeroPad2d(1)?, Conv2d 3x3 (no bias), BatchNorm2d, ReLU] groups (:154-169, :171-175, :200-209): the
            explicit zero pad + pad-0 conv of the strided entries is the same pad-1 convolution.  gate / resid: the SFM step
            gate * cbr(t) + resid folded into the last BatchNorm + ReLU."""
            mods, k = list(seq), 0
            while k < len(mods):
                if isinstance(mods[k], nn.ZeroPad2d):
                    k += 1
                conv, bn = mods[k], mods[k + 1]
                last = k + 3 >= len(mods)
                if last and gate is not None and resid is t and conv.stride[0] == 1 and conv.kernel_size[0] == 3:
                    t = ct.sfm_step(t, conv.weight, bn, gate)            # the SFM step as one autograd node
                else:
                    z, partials = ct.conv(t, conv.weight, conv.stride[0], stats=True)
                    t = ct.bn_relu(z, bn, gate=gate if last else None, resid=resid if last else None, partials=partials)
                k += 3
            return t

        def gate(y, uses):
            """SpatialAttention on the scale stream (spatial_attention.py:57-63) with batch statistics, forward and backward on
            hvpr_spatial_gate_train_*: ChannelPool -> conv3x3 2 -> 1 -> BatchNorm2d(1) -> sigmoid.  The reference calls the module
            once per SFM step and stream with the SAME input (:250-257): the values are identical every time, so the gate is
            computed once per level (its gradient accumulates over the uses through autograd) and the BatchNorm's running
            statistics receive the `uses` identical updates in closed form."""
            sp = self.attention.spatial
            g, mean, var = ct.spatial_gate_train(y, sp.conv.weight, sp.conv.bias, sp.norm.weight, sp.norm.bias, sp.norm.eps)
            ct.update_running_repeated(sp.norm, mean, var, ct.global_count(y.numel() // y.shape[-1], y.device), uses)
            return g                                                                       # (N,H,W,1)

        x, xp = nhwc(data_dict["spatial_features"]), nhwc(data_dict["spatial_features_point"])
        y = nhwc(data_dict["spatial_scale_features"])
        ups, ups_p = [], []
        for i in range(len(self.blocks)):
            x = cbr(self.blocks[i], x)
            xp = cbr(self.blocks[i], xp)
            y = cbr(self.scale_layers[i], y)
            xa, xpa = x, xp
            nsfm = self.sfm_layer_nums[i]
            if nsfm > 0:
                g = gate(y, 2 * nsfm)
                for _ in range(nsfm):
                    xa = cbr(self.sfmblocks_down[i], xa, gate=g, resid=xa)
                    xpa = cbr(self.sfmblocks_down[i], xpa, gate=g, resid=xpa)
            de = self.deblocks[i]
            ups.append(ct.deconv(xa, de[0].weight))
            ups_p.append(ct.deconv(xpa, de[0].weight))
        # BatchNorm + ReLU of the three branches write straight into their slices of the concatenation (:262-279).  The two streams share
        # the BatchNorm modules: statistics per stream, running statistics updated by the first stream's call and then the second's, as
        # the reference's two passes do
        bns = [de[1] for de in self.deblocks]
        data_dict["spatial_features_2d"] = ct.bn_relu_cat(ups, bns).permute(0, 3, 1, 2)          # (B, 384, H, W), channels_last
        data_dict["spatial_features_point_2d"] = ct.bn_relu_cat(ups_p, bns).permute(0, 3, 1, 2)
        return data_dict

    def _head(self, plan, x, y, out, level, x_out={}, y_out=None):
        """The whole trunk and the branches of the levels below `level`; x_out[i] / y_out receive the trunk output of level i / the
        scale output of level - 1."""
        fork = _Fork(self._streams(y.device))
        for lv in plan.levels:
            x = _trunk(lv, x, out=x_out.get(lv.index))
            if lv.index < level:
                y = _branch(lv, x, y, out, fork, y_out=y_out if lv.index == level - 1 else None)
        fork.join()

    def forward(self, data_dict):
        if self.training:
            return self._forward_train(data_dict)
        x, y = _nhwc(data_dict["spatial_features"]), _nhwc(data_dict["spatial_scale_features"])
        plan = self._fold.get(y.device, self._build_plan)
        out = self._canvas(x)
        if plan.planes:
            x = kernels.split_bf16(x, plan.planes)        # the trunk runs in split-bf16 form from here on
        self._head(plan, x, y, out, len(plan.levels))
        data_dict["spatial_features_2d"] = out.permute(0, 3, 1, 2)   # (B, 384, H, W), channels_last
        return data_dict

    def forward_head(self, spatial, scale, split):
        """First half of the eval forward on the boundary buffers `split` (split_buffers) — the frame pipeline overlaps the halves of
        neighbouring frames: the whole trunk and the branches of the levels below L = split["level"].  Writes split["x"][i] = the trunk
        output of every level i >= L, split["y"] = the scale output of level L - 1, and its slices of split["out"] = the concat."""
        y = _nhwc(scale)
        plan = self._fold.get(y.device, self._build_plan)
        assert not plan.planes, "the split forward runs the fp32 kernels"
        self._head(plan, _nhwc(spatial), y, split["out"], split["level"], split["x"], split["y"])

    def forward_tail(self, split):
        """Second half: the branches of the levels >= split["level"] (reads split["x"], split["y"]; finishes split["out"]).  Returns
        spatial_features_2d, a view of split["out"]."""
        y, out = split["y"], split["out"]
        plan = self._fold.get(y.device, self._build_plan)
        assert not plan.planes, "the split forward runs the fp32 kernels"
        # the caller runs this half on a forked stream of its capture: forking again from it (a second level of stream forks inside
        # one hipGraph capture) crashed hipStreamEndCapture on this ROCm build, so its branches stay in line
        fork = _Fork([])
        for lv in plan.levels[split["level"]:]:
            y = _branch(lv, split["x"][lv.index], y, out, fork)
        fork.join()
        return out.permute(0, 3, 1, 2)                               # (B, 384, H, W), channels_last

    def split_buffers(self, batch_size, H, W, device, level=None):
        """Boundary buffers of forward_head / forward_tail for canvases of (H, W): x[i] (trunk output of every level i >= level), y
        (scale output of level - 1), out (the concat).  level defaults to the last one; >= 1."""
        n_lv = len(self.blocks)
        if level is None:
            level = n_lv - 1
        assert 1 <= level <= n_lv - 1
        h, w, hw = H, W, []
        for s in self.layer_strides:
            h, w = (h + 2 - 3) // s + 1, (w + 2 - 3) // s + 1
            hw.append((h, w))
        cy = self.scale_layers[level - 1][1].weight.shape[0]
        us0 = int(self.upsample_strides[0])
        mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        return {"level": level,
                "x": {i: mk(batch_size, hw[i][0], hw[i][1], self.blocks[i][1].weight.shape[0]) for i in range(level, n_lv)},
                "y": mk(batch_size, hw[level - 1][0], hw[level - 1][1], cy),
                "out": mk(batch_size, hw[0][0] * us0, hw[0][1] * us0, self.num_bev_features)}


class BaseBEVBackbone(_BEVTrunk):
    """Plain PointPillars' backbone — base_bev_backbone.py:6-113: per level a strided entry convolution and LAYER_NUMS[i] more, all
    3x3 + BatchNorm + ReLU, then a ConvTranspose2d (kernel == stride) + BatchNorm + ReLU into the level's slice of the concat.

    The eval forward is a plan over the same fp32 ops as BaseBEVBackbone_Scale's trunk and deconvolutions (_Level with no scale
    stream, gate or SFM steps), built once per fold and run in line on the current stream: HVPR_BEV_STREAMS is not consulted, there
    are no branches to overlap.  fp32 only.  Settings the ops do not take raise at construction."""

    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        layer_nums, strides, filters = (list(model_cfg.get(k, None) or []) for k in ("LAYER_NUMS", "LAYER_STRIDES", "NUM_FILTERS"))
        if not (len(layer_nums) == len(strides) == len(filters)) or not layer_nums:
            raise ValueError("hvpr_amd: BaseBEVBackbone needs LAYER_NUMS, LAYER_STRIDES and NUM_FILTERS of one length >= 1")
        up_strides = list(model_cfg.get("UPSAMPLE_STRIDES", None) or [])
        up_filters = list(model_cfg.get("NUM_UPSAMPLE_FILTERS", None) or [])
        if not up_strides:
            raise ValueError("hvpr_amd: BaseBEVBackbone is built with UPSAMPLE_STRIDES (one deblock per level writes the concat)")
        if len(up_strides) != len(up_filters):
            raise ValueError("hvpr_amd: UPSAMPLE_STRIDES and NUM_UPSAMPLE_FILTERS differ in length")
        if len(up_strides) > len(layer_nums):
            raise ValueError("hvpr_amd: BaseBEVBackbone is built for one deblock per level (no extra final deblock)")
        if len(up_strides) < len(layer_nums):
            raise ValueError("hvpr_amd: BaseBEVBackbone needs an UPSAMPLE_STRIDES entry for every level")
        for s in up_strides:
            if s < 1 or int(s) != s:
                raise ValueError(f"hvpr_amd: BaseBEVBackbone takes integer UPSAMPLE_STRIDES (ConvTranspose2d with kernel == stride), got {s}")
        for s in strides:
            if s not in (1, 2):
                raise ValueError(f"hvpr_amd: BaseBEVBackbone takes LAYER_STRIDES of 1 or 2, got {s}")
        precision = model_cfg.get("CONV_PRECISION", "fp32")
        if precision != "fp32":
            raise ValueError(f"hvpr_amd: BaseBEVBackbone runs the fp32 convolutions only, CONV_PRECISION is {precision!r}")
        cin = [input_channels] + filters[:-1]
        if any(c % 8 for c in cin + filters) or any(c % 4 for c in up_filters):
            raise ValueError("hvpr_amd: the convolutions take input channels in multiples of 8 and output channels in multiples of 4 "
                             f"(input {input_channels}, NUM_FILTERS {filters}, NUM_UPSAMPLE_FILTERS {up_filters})")
        self.layer_strides, self.layer_nums = [int(s) for s in strides], [int(n) for n in layer_nums]
        self.upsample_strides, self.up_filters = [int(s) for s in up_strides], [int(c) for c in up_filters]
        self.blocks, self.deblocks = nn.ModuleList(), nn.ModuleList()
        for i in range(len(layer_nums)):
            self.blocks.append(_block(cin[i], filters[i], self.layer_strides[i], self.layer_nums[i]))
            self.deblocks.append(_deblock(filters[i], up_filters[i], self.upsample_strides[i]))
        self.num_bev_features = sum(self.up_filters)

    def _build_plan(self):
        """Every level's trunk and deconvolution on the fp32 kernels, no branch."""
        return _Plan([_Level(i, trunk, None, None, [], _deconv_f32(de), coff) for i, trunk, de, coff in self._trunks(_conv_f32)], 0)

    def forward(self, data_dict):
        if self.training:
            raise NotImplementedError("hvpr_amd: BaseBEVBackbone has no training forward (plain PointPillar is eval only; train MixAnchor_Memory)")
        x = _nhwc(data_dict["spatial_features"])
        plan = self._fold.get(x.device, self._build_plan)
        out = self._canvas(x)
        for lv in plan.levels:
            x = _trunk(lv, x)
            kernels.conv2d_nhwc(x, lv.deconv, out=out, out_coff=lv.coff, use_table=True)
        data_dict["spatial_features_2d"] = out.permute(0, 3, 1, 2)   # (B, sum(NUM_UPSAMPLE_FILTERS), H, W), channels_last
        return data_dict


__all__ = {
    "BaseBEVBackbone_Scale": BaseBEVBackbone_Scale,
    "BaseBEVBackbone": BaseBEVBackbone,
}
