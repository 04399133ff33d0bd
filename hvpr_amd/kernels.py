"""Tensor-level wrappers over the C-ABI (include/hvpr_amd.h): torch is used for device memory and streams only.

Every wrapper hands its tensors and the current HIP stream to _lib.call, which checks each tensor against the header's
parameter (device, dtype, contiguity), passes its pointer and raises on a non-zero status.  There is no CPU path: CPU
tensors are rejected.  Host-side arguments (pinned host tensors, numpy and ctypes arrays) go as raw addresses.
"""
import ctypes
import os

import numpy as np
import torch

from ._lib import call, check, lib  # noqa: F401  (check: callers reach it as kernels.check)


def _stream():
    try:
        return torch.cuda.current_stream().cuda_stream
    except RuntimeError as e:        # no usable GPU: say so in the words every other refusal of a CPU run uses
        raise RuntimeError(f"hvpr_amd needs a GPU (the HIP path has no CPU fallback): {e}") from e


# ------------------------------------------------------------------------------------------------ voxelizer
class VoxelizeWorkspace:
    """Persistent device workspace of the voxelizer (two cell maps + per-point scratch), sized for up to `batch`
    frames / `n_points` points per call."""

    def __init__(self, batch, n_points, grid, device):
        self.key = (int(batch), int(n_points), tuple(int(g) for g in grid), torch.device(device))
        nx, ny, nz = self.key[2]
        nbytes = lib().hvpr_voxelize_workspace_bytes(batch, n_points, nx, ny, nz)
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.reset()

    def reset(self):
        batch, n_points, (nx, ny, nz), _ = self.key
        call("hvpr_voxelize_workspace_reset", self.buf, self.buf.numel(), batch, n_points, nx, ny, nz, _stream())

    def status(self):
        """SYNCHRONISES the current stream; raises when a one-launch index kernel (encode_fwd(index_mode=1)) gave up a wait on this
        workspace since its last reset (that call and every later one reported zero pillars): reset() it."""
        batch, n_points, (nx, ny, nz), _ = self.key
        call("hvpr_voxelize_workspace_status", self.buf, self.buf.numel(), batch, n_points, nx, ny, nz, _stream())


def voxelize(points, frame_offsets, batch, point_cloud_range, voxel_size, grid, max_points, max_voxels, workspace,
             xyz_col=0, n_feat=None, cap_mode=0, capacity=None):
    """points (N, stride) f32 cuda; frame_offsets (batch+1,) i32 cuda.

    Returns voxels (cap, P, n_feat) f32, coords (cap, 4) i32 [b,z,y,x], num_points (cap,) i32,
    voxel_offsets (batch+1,) i32 — rows past voxel_offsets[batch] are unspecified.
    """
    n, stride = points.shape
    n_feat = stride - xyz_col if n_feat is None else n_feat
    if capacity is None:
        capacity = min(n, batch * max_voxels)
    dev = points.device
    voxels = torch.empty((capacity, max_points, n_feat), dtype=torch.float32, device=dev)
    coords = torch.empty((capacity, 4), dtype=torch.int32, device=dev)
    num = torch.empty((capacity,), dtype=torch.int32, device=dev)
    offs = torch.empty((batch + 1,), dtype=torch.int32, device=dev)
    nx, ny, nz = [int(g) for g in grid]
    lo = [float(torch.tensor(v, dtype=torch.float32)) for v in point_cloud_range[:3]]
    vs = [float(torch.tensor(v, dtype=torch.float32)) for v in voxel_size]
    if workspace.key[0] < batch or workspace.key[1] < n:
        raise ValueError("voxelize workspace too small for this call")
    call("hvpr_voxelize_f32", points, n, stride, xyz_col, n_feat, frame_offsets, batch, lo[0], lo[1], lo[2], vs[0], vs[1], vs[2], nx, ny,
         nz, int(max_points), int(max_voxels), int(cap_mode), voxels, coords, num, offs, capacity, workspace.buf, workspace.buf.numel(),
         workspace.key[0], workspace.key[1], _stream())
    return voxels, coords, num, offs


# ------------------------------------------------------------------------------------------------ VFE
def pillar_vfe_fwd(voxels, num_points, coords, folded, voxel_size, offsets, m_device=None, want_mask=True):
    """folded: dict w0,b0,w1,b1,ws0,bs0,ws1,bs1 (f32 cuda, BN folded). Returns (pillar, scale, mask|None)."""
    M, P, C = voxels.shape
    if C != 4:
        raise ValueError("hvpr_pillar_vfe_fwd_f32 is built for 4 raw point features")
    dev = voxels.device
    pf = torch.empty((M, 64), dtype=torch.float32, device=dev)
    sf = torch.empty((M, 32), dtype=torch.float32, device=dev)
    mask = torch.empty((M, P, 1), dtype=torch.float32, device=dev) if want_mask else None
    call("hvpr_pillar_vfe_fwd_f32", voxels, num_points, coords, M, P, m_device, float(voxel_size[0]), float(voxel_size[1]),
         float(voxel_size[2]), float(offsets[0]), float(offsets[1]), float(offsets[2]), folded["w0"], folded["b0"], folded["w1"],
         folded["b1"], folded["ws0"], folded["bs0"], folded["ws1"], folded["bs1"], pf, sf, mask, _stream())
    return pf, sf, mask


def pillar_vfe_plain_fwd(voxels, num_points, coords, w, b, voxel_size, offsets, m_device=None, want_mask=True):
    """Plain PointPillars' one-layer pillar encoder (hvpr_pillar_vfe_plain_fwd_f32).  w (c_out, 10), b (c_out,): the folded
    Linear + BatchNorm (f32 cuda), c_out in {32, 64, 128}.  Returns (pillar (M, c_out), mask (M, P, 1)|None)."""
    M, P, C = voxels.shape
    if C != 4:
        raise ValueError("hvpr_pillar_vfe_plain_fwd_f32 is built for 4 raw point features")
    if w.dim() != 2 or w.shape[1] != 10 or tuple(b.shape) != (w.shape[0],):
        raise ValueError("hvpr_pillar_vfe_plain_fwd_f32 takes w (c_out, 10) and b (c_out,)")
    dev = voxels.device
    pf = torch.empty((M, w.shape[0]), dtype=torch.float32, device=dev)
    mask = torch.empty((M, P, 1), dtype=torch.float32, device=dev) if want_mask else None
    call("hvpr_pillar_vfe_plain_fwd_f32", voxels, num_points, coords, M, P, m_device, float(voxel_size[0]), float(voxel_size[1]),
         float(voxel_size[2]), float(offsets[0]), float(offsets[1]), float(offsets[2]), w, b, int(w.shape[0]), pf, mask, _stream())
    return pf, mask


# ------------------------------------------------------------------------------------------------ memory + scatter
class PackedBank:
    """Memory bank with its streaming copy for the read-out kernel (hvpr_memory_bank_pack_f32): IEEE fp16 tiles in the matrix-core
    operand layout ([tile of 16 items][channel half][64 lanes] x 8 fp16, 1 KB contiguous per load instruction) + the 64
    channel maxima max_j |W_jc| that bound the pre-filter's rounding error.  The fp32 rows stay next to it: candidates are
    re-checked and the k selected rows are read in exact fp32."""

    def __init__(self, weight):
        w = weight.detach().float().contiguous()
        if w.dim() != 2 or w.shape[1] != 64:
            raise ValueError("PackedBank: (n_items, 64) memory bank expected")
        self.n_items = int(w.shape[0])
        self.shape = w.shape
        self.rows = w                 # row-major copy: the k selected rows are gathered from it
        self.data = torch.empty(lib().hvpr_memory_bank_packed_floats(self.n_items), dtype=torch.float32, device=w.device)
        call("hvpr_memory_bank_pack_f32", w, self.n_items, self.data, _stream())


def _bank_args(bank):
    """(row-major pointer, packed pointer, n_items) of a PackedBank; a plain (n_items, 64) tensor is packed here (callers that
    reuse a bank pack it once themselves)."""
    if not isinstance(bank, PackedBank):
        bank = PackedBank(bank)
    return bank.rows, bank.data, bank.n_items


def memory_readout_fwd(f, bank, k, m_device=None, want_idx=False):
    M, C = f.shape
    out = torch.empty((M, C), dtype=torch.float32, device=f.device)
    idx = torch.empty((M, k), dtype=torch.int32, device=f.device) if want_idx else None
    call("hvpr_memory_readout_fwd_f32", f, M, m_device, *_bank_args(bank), int(k), out, idx, _stream())
    return (out, idx) if want_idx else out


_SEG_CHUNK = 32      # edges per first-level sum of segment_sum_rows


def edges_by_destination(dst, n_dst):
    """The edges e -> dst[e] of a scatter, grouped by destination for hvpr_segment_sum_rows_f32.  Returns (order, chunk_ptr, dest_ptr):
    order i32 lists the edge ids destination by destination, inside a destination by ascending edge id (a STABLE sort: the summation
    order is a fixed function of the index tensor, so the scattering gradients are reproducible bit for bit, which float atomics are
    not).  A destination's run of edges is cut into chunks of _SEG_CHUNK: chunk_ptr i32 [n_chunks_max + 1] are the chunk boundaries
    inside `order`, dest_ptr i32 [n_dst + 1] the chunks of each destination — a point picked by 2000 pillars becomes 63 short sums on
    63 waves and one sum of 63 partials instead of one 2000-term loop on one wave.  Everything stays on the device: the chunk count
    is bounded by E / _SEG_CHUNK + min(n_dst, E) (n_chunks_max is that bound plus one spare chunk, E counting the dropped edges too),
    the unused tail of chunk_ptr is empty chunks.  Destinations outside [0, n_dst)
    are dropped (they sort to the two ends)."""
    dst = dst.reshape(-1).to(torch.int64)
    dev = dst.device
    E = dst.numel()
    n_max = E // _SEG_CHUNK + min(n_dst, E) + 1
    if E == 0:
        z = torch.zeros(1, dtype=torch.int32, device=dev)
        return torch.zeros(0, dtype=torch.int32, device=dev), z.expand(n_max + 1).contiguous(), z.expand(n_dst + 1).contiguous()
    order = torch.argsort(dst, stable=True)
    sdst = dst[order].contiguous()
    rowptr = torch.searchsorted(sdst, torch.arange(n_dst + 1, dtype=torch.int64, device=dev))   # edges of d: rowptr[d] .. rowptr[d+1]
    end_live = rowptr[n_dst:]                                                   # (1,)
    pos = torch.arange(E, dtype=torch.int64, device=dev)
    live = (sdst >= 0) & (sdst < n_dst)
    first = rowptr[sdst.clamp(0, n_dst - 1)]                                    # first edge of this edge's destination
    head = live & (((pos - first) % _SEG_CHUNK) == 0)                           # this edge opens a chunk
    csum = torch.cumsum(head.to(torch.int64), 0)
    cid, total = csum - 1, csum[-1:]                                            # chunk of every live edge; number of chunks
    chunk_ptr = end_live.expand(n_max + 1).clone()                              # chunks past the last one: empty, at the end
    chunk_ptr.scatter_(0, torch.where(head, cid, torch.full_like(cid, n_max)), torch.where(head, pos, end_live.expand(E)))
    # chunks of destination d: from the chunk its first edge opens (for an empty d: the next destination's) to the next one's
    dest_ptr = torch.where(rowptr < end_live, cid[rowptr.clamp(max=E - 1)], total.expand(n_dst + 1))
    return order.to(torch.int32), chunk_ptr.to(torch.int32), dest_ptr.to(torch.int32)


def segment_sum_rows(src, src_off, C, edge_row, edge_w, chunk_ptr, dest_ptr, n_dst):
    """dst (n_dst, C): dst[d] = sum over d's edges, in the order given, of edge_w[e] * src[edge_row[e], off : off + C] — two passes of
    hvpr_segment_sum_rows_f32: per chunk of <= _SEG_CHUNK edges, then per destination over its chunks (fixed order: reproducible)."""
    n_chunks = chunk_ptr.numel() - 1
    part = torch.empty((n_chunks, C), dtype=torch.float32, device=src.device)
    call("hvpr_segment_sum_rows_f32", src, src.shape[-1], int(src_off), int(C), edge_row, edge_w, chunk_ptr, int(n_chunks), part, int(C),
         _stream())
    dst = torch.empty((n_dst, C), dtype=torch.float32, device=src.device)
    call("hvpr_segment_sum_rows_f32", part, int(C), 0, int(C), None, None, dest_ptr, int(n_dst), dst, int(C), _stream())
    return dst


class EdgePlan:
    """The edges e -> idx[e] of a scatter into n_dst rows, owned in one place: edges_by_destination's (order, chunk_ptr, dest_ptr) —
    one stable argsort + a handful of scans — made on first use (build() forces it), kept, and shared by every gradient that
    scatters along the SAME index tensor; sum_rows is segment_sum_rows over it.  EdgePlan(dst, n_dst): dst is an integer tensor of
    any shape, read flat, edge e goes to row dst[e] (rows outside [0, n_dst) are dropped)."""

    def __init__(self, dst, n_dst):
        self.idx, self.n_dst, self._per_batch = dst, int(n_dst), None
        self._plan, self._rows, self._i32 = None, {}, None

    @classmethod
    def batched(cls, idx, n_per_batch):
        """idx (B, ...) picks among n_per_batch rows of ITS sample: edge e of sample b goes to row b * n_per_batch + idx[e] (the
        backward of the point stream's gathers).  Depends on idx only, so the index plan of a batch (PointNet2MSG.index_plan,
        computed ahead on a side stream) carries it built and the backward does not have to sort."""
        plan = cls(idx, idx.shape[0] * int(n_per_batch))
        plan._per_batch = int(n_per_batch)
        return plan

    def build(self):
        if self._plan is None:
            dst = self.idx
            if self._per_batch is not None:
                B = dst.shape[0]
                dst = dst.reshape(B, -1).to(torch.int64) + torch.arange(B, device=dst.device, dtype=torch.int64).view(B, 1) * self._per_batch
            self._plan = edges_by_destination(dst, self.n_dst)
        return self

    def tensors(self):
        """Every device tensor the plan has made so far (a consumer on another stream than the builder's records them)."""
        made = list(self._plan or ()) + list(self._rows.values())
        return made if self._i32 is None else made + [self._i32]

    def idx32(self):
        """idx as the contiguous i32 tensor the forward kernels read (one copy for every op that shares the plan)."""
        if self._i32 is None:
            self._i32 = self.idx.to(torch.int32).contiguous()
        return self._i32

    def edge_rows(self, per=1):
        """i32, in the plan's order: the source row e // per of edge e (per = 1: one edge per source row; 3: three_interpolate's
        neighbours of a row; k: the picks of a pillar).  Cached per `per`."""
        if per not in self._rows:
            order = self.build()._plan[0]
            self._rows[per] = order if per == 1 else torch.div(order, per, rounding_mode="floor")
        return self._rows[per]

    def edge_weights(self, weights):
        """weights holds one value per edge in edge-id order (any shape): the same values in the plan's order."""
        return torch.index_select(weights.reshape(-1), 0, self.build()._plan[0])

    def sum_rows(self, src, src_off=0, C=None, *, per=1, weights=None):
        """(n_dst, C): row d = the sum over d's edges, in ascending edge id, of weights[e] * src[e // per, src_off : src_off + C]
        (weights None: 1; C None: up to the row's end) — a fixed order, no float atomics: the same bits every run."""
        _, chunk_ptr, dest_ptr = self.build()._plan
        C = src.shape[-1] - src_off if C is None else C
        return segment_sum_rows(src, src_off, C, self.edge_rows(per), None if weights is None else self.edge_weights(weights),
                                chunk_ptr, dest_ptr, self.n_dst)


def attend_rows(q, rows, idx=None, k=None):
    """hvpr_attend_rows_fwd_f32: w[m] = softmax_j <q[m], rows[r(m,j)]>, out[m] = sum_j w[m,j] rows[r(m,j)] without the gathered
    (M, k, 64) tensor.  q (M, 64), rows (N, 64) f32; idx (M, k) i32 picks rows of the table, idx=None is the dense form over
    rows = an (M*k, 64) tensor (k given).  Returns (out (M, 64), w (M, k)); no autograd here (map_to_bev._AttendRows)."""
    if idx is not None:
        if idx.dim() != 2 or (k is not None and int(k) != idx.shape[1]):
            raise ValueError("hvpr_amd: attend_rows needs idx of shape (M, k)")
        k = idx.shape[1]
    elif k is None:
        raise ValueError("hvpr_amd: attend_rows without idx needs k")
    M, C = q.shape
    if rows.dim() != 2 or rows.shape[1] != C or (idx is not None and idx.shape[0] != M):
        raise ValueError("hvpr_amd: attend_rows needs q (M, C), rows (N, C) and idx (M, k)")
    out = torch.empty((M, C), dtype=torch.float32, device=q.device)
    w = torch.empty((M, int(k)), dtype=torch.float32, device=q.device)
    call("hvpr_attend_rows_fwd_f32", q, M, rows, rows.shape[0], idx, int(k), C, out, w, _stream())
    return out, w


def scatter_workspace(batch, nx, ny, device):
    """Idle cell map (-1 everywhere); every call returns it to idle."""
    n = lib().hvpr_scatter_workspace_bytes(batch, nx, ny) // 4
    return torch.full((n,), -1, dtype=torch.int32, device=device)


def scatter_bev_fwd(pillar, memory, scale, coords, batch, nx, ny, workspace, m_device=None):
    """Returns spatial (B, Cp+Cm, ny, nx) and spatial_scale (B, Cs, ny, nx) in channels_last memory format."""
    M, cp = pillar.shape
    cm = 0 if memory is None else memory.shape[1]
    cs = 0 if scale is None else scale.shape[1]
    dev = pillar.device
    spatial = torch.empty((batch, ny, nx, cp + cm), dtype=torch.float32, device=dev)
    spatial_scale = torch.empty((batch, ny, nx, cs), dtype=torch.float32, device=dev) if cs else None
    call("hvpr_scatter_bev_fwd_f32", pillar, cp, memory, cm, scale, cs, coords, M, m_device, batch, nx, ny, spatial, spatial_scale,
         workspace, workspace.numel() * 4, _stream())
    spatial = spatial.permute(0, 3, 1, 2)
    if spatial_scale is not None:
        spatial_scale = spatial_scale.permute(0, 3, 1, 2)
    return spatial, spatial_scale


# ------------------------------------------------------------------------------------------------ split-bf16 convolutions
class PackedConvBf3:
    """Weights split into `planes` bf16 planes, layout [taps, Cin/8, planes, cout_pad, 8] (BatchNorm scale folded).  up is None: a 3x3
    convolution (pack_conv_bf3) whose output is split-bf16 again (out_split) or fp32; up = s: a ConvTranspose2d with kernel ==
    stride == s as a 1x1 GEMM (pack_deconv_bf3), fp32 output."""

    def __init__(self, w, bias, cin, cout, cout_pad, stride, relu, tile_cfg, planes, up=None, out_split=True):
        self.w, self.bias, self.cin, self.cout, self.cout_pad = w, bias, cin, cout, cout_pad
        self.stride, self.relu, self.tile_cfg, self.planes, self.up, self.out_split = stride, relu, tile_cfg, planes, up, out_split

    def fp32_output(self):
        """The same layer (shared weight image) writing fp32 NHWC: the hand-over from a split-bf16 chain to an fp32 kernel."""
        return PackedConvBf3(self.w, self.bias, self.cin, self.cout, self.cout_pad, self.stride, self.relu, self.tile_cfg, self.planes,
                             out_split=False)


def _planes_of(x, planes):
    out, r = [], x
    for _ in range(planes):
        h = r.to(torch.bfloat16)
        out.append(h)
        r = r - h.float()
    return out


def pack_conv_bf3(weight, scale=None, shift=None, stride=1, relu=True, tile_cfg=0, planes=2):
    cout, cin, kh, kw = weight.shape
    assert kh == kw == 3 and cin % 16 == 0 and cout % 4 == 0 and planes in (2, 3)
    w = weight.detach().float()
    if scale is not None:
        w = w * scale.view(-1, 1, 1, 1)
    cout_pad = (cout + 63) // 64 * 64
    wp = torch.zeros((9, cin // 8, planes, cout_pad, 8), dtype=torch.bfloat16, device=w.device)
    for k, part in enumerate(_planes_of(w, planes)):       # (Cout, Cin, 3, 3) -> tap, chunk, ci, co -> tap, chunk, co, ci
        wp[:, :, k, :cout, :] = part.permute(2, 3, 1, 0).reshape(9, cin // 8, 8, cout).permute(0, 1, 3, 2)
    b = torch.zeros((cout_pad,), dtype=torch.float32, device=w.device)
    if shift is not None:
        b[:cout] = shift.detach().float()
    return PackedConvBf3(wp.contiguous(), b, cin, cout, cout_pad, stride, relu, tile_cfg, planes)


def pack_deconv_bf3(weight, scale, shift, relu=True, planes=2):
    """ConvTranspose2d weight (Cin, Cout, s, s), kernel == stride == s -> 1x1 GEMM with s*s*Cout columns, split planes."""
    cin, cout, s, s2 = weight.shape
    assert s == s2 and cin % 64 == 0 and cout % 4 == 0 and planes in (2, 3)
    w = weight.detach().float() * scale.view(1, -1, 1, 1)
    cols = s * s * cout
    cout_pad = (cols + 63) // 64 * 64
    g = w.permute(0, 2, 3, 1).reshape(cin, cols)                          # column = (ky*s + kx)*Cout + co
    wp = torch.zeros((1, cin // 8, planes, cout_pad, 8), dtype=torch.bfloat16, device=w.device)
    for k, part in enumerate(_planes_of(g, planes)):
        wp[0, :, k, :cols, :] = part.reshape(cin // 8, 8, cols).permute(0, 2, 1)
    b = torch.zeros((cout_pad,), dtype=torch.float32, device=w.device)
    b[:cols] = shift.detach().float().repeat(s * s)
    return PackedConvBf3(wp.contiguous(), b, cin, cout, cout_pad, 1, relu, 1, planes, up=s)


def deconv_nhwc_bf3(xs, pc, out, out_coff=0):
    """xs split-bf16 NHWC (N,H,W,Cin/8,planes,8) -> fp32 into out[..., out_coff:out_coff+Cout] at pc.up x the resolution."""
    N, H, W, groups, planes, _ = xs.shape
    assert groups * 8 == pc.cin and planes == pc.planes and xs.is_contiguous()
    assert out.shape[:3] == (N, H * pc.up, W * pc.up) and out.is_contiguous() and out.dtype == torch.float32
    call("hvpr_deconv_nhwc_bf16x3", xs, N, H, W, pc.cin, pc.w, pc.bias, pc.cout, pc.cout_pad, pc.up, 1 if pc.relu else 0, out,
         out.shape[-1], out_coff, planes, _stream())
    return out


def split_bf16(x, planes=2):
    """fp32 NHWC (..., C), C % 8 == 0 -> split-bf16 NHWC as a bf16 tensor (..., C/8, planes, 8)."""
    assert x.is_contiguous() and x.shape[-1] % 8 == 0 and x.dtype == torch.float32
    out = torch.empty((*x.shape[:-1], x.shape[-1] // 8, planes, 8), dtype=torch.bfloat16, device=x.device)
    call("hvpr_split_bf16_f32", x, x.numel(), planes, out, _stream())
    return out


def unsplit_bf16(xs):
    """split-bf16 NHWC (..., C/8, planes, 8) -> fp32 NHWC (..., C)."""
    assert xs.is_contiguous() and xs.dtype == torch.bfloat16 and xs.shape[-1] == 8
    planes = xs.shape[-2]
    out = torch.empty((*xs.shape[:-3], xs.shape[-3] * 8), dtype=torch.float32, device=xs.device)
    call("hvpr_unsplit_bf16_f32", xs, out.numel(), planes, out, _stream())
    return out


def conv2d_nhwc_bf3(xs, pc, out_split=True, gate=None, resid=None):
    """xs: split-bf16 NHWC (N,H,W,Cin/8,planes,8).  Returns split-bf16 NHWC (out_split) or fp32 NHWC (N,OH,OW,Cout)."""
    N, H, W, groups, planes, _ = xs.shape
    cin = groups * 8
    assert cin == pc.cin and planes == pc.planes and xs.is_contiguous()
    OH, OW = (H + 2 - 3) // pc.stride + 1, (W + 2 - 3) // pc.stride + 1
    if out_split:
        assert pc.cout % 8 == 0
        out = torch.empty((N, OH, OW, pc.cout // 8, planes, 8), dtype=torch.bfloat16, device=xs.device)
    else:
        out = torch.empty((N, OH, OW, pc.cout), dtype=torch.float32, device=xs.device)
    call("hvpr_conv2d_nhwc_bf16x3", xs, N, H, W, cin, pc.w, pc.bias, pc.stride, pc.cout, pc.cout_pad, 1 if pc.relu else 0, gate, resid,
         0 if resid is None else resid.shape[3] * 8, out, 1 if out_split else 0, pc.cout, 0, pc.tile_cfg, planes, _stream())
    return out


def memory_scatter_fwd(pillar, scale, coords, bank, k, batch, nx, ny, workspace, m_device=None, out=None):
    """Fused a3+a4 (64+64+32 channels): returns memory_features (M,64), spatial (B,128,ny,nx), spatial_scale (B,32,ny,nx).
    `out` = (spatial, spatial_scale) as returned by an earlier call: write into those canvases instead of new ones."""
    M = pillar.shape[0]
    dev = pillar.device
    mem = torch.empty((M, 64), dtype=torch.float32, device=dev)
    if out is not None:
        spatial, spatial_scale = (o.permute(0, 2, 3, 1) for o in out)
        if spatial.shape != (batch, ny, nx, 128) or spatial_scale.shape != (batch, ny, nx, 32) or not spatial.is_contiguous() \
                or not spatial_scale.is_contiguous():
            raise ValueError("memory_scatter_fwd: `out` canvases do not match this call")
    else:
        spatial = torch.empty((batch, ny, nx, 128), dtype=torch.float32, device=dev)
        spatial_scale = torch.empty((batch, ny, nx, 32), dtype=torch.float32, device=dev)
    if pillar.shape[1] != 64 or scale.shape[1] != 32 or bank.shape[1] != 64:
        raise ValueError("memory_scatter_fwd is specialised for 64 pillar / 64 memory / 32 scale channels")
    call("hvpr_memory_scatter_fwd_f32", pillar, scale, coords, M, m_device, *_bank_args(bank), int(k), batch, nx, ny, mem, spatial,
         spatial_scale, workspace, workspace.numel() * 4, _stream())
    return mem, spatial.permute(0, 3, 1, 2), spatial_scale.permute(0, 3, 1, 2)


def frame_offsets(points, batch):
    """(batch+1,) i32 frame offsets of a collated (N, C) point tensor whose column 0 is the batch index (one launch)."""
    offs = torch.empty((batch + 1,), dtype=torch.int32, device=points.device)
    call("hvpr_frame_offsets_f32", points, points.shape[0], points.shape[1], int(batch), offs, _stream())
    return offs


def encode_fwd(points, frame_offsets, batch, point_cloud_range, voxel_size, grid, max_points, max_voxels, workspace, folded,
               offsets, bank, k, xyz_col=0, cap_mode=0, capacity=None, want_voxels=True, want_mask=True, out=None, state=None,
               index_mode=0):
    """a1..a4 fused (hvpr_encode_fwd_f32): raw points -> canvases in five launches (three with index_mode=1: the index phase as ONE
    launch, for a caller with a single encode lane per device — include/hvpr_amd.h), bit-identical to voxelize ->
    pillar_vfe_fwd -> memory_scatter_fwd.  Returns a dict with voxels|None, coords, num_points, voxel_offsets,
    pillar_features, pillar_scale_features, pillar_mask|None, memory_features, spatial (B,128,ny,nx), spatial_scale
    (B,32,ny,nx) (channels_last).  `out` = (spatial, spatial_scale) of an earlier call: write into those canvases.
    `state` (with `out`): the uint8 (B*ny*nx,) occupancy that travels with those canvases (see canvas_buffers): only the
    cells the previous call left non-zero are cleared instead of the whole 47 MB."""
    n, stride = points.shape
    n_feat = stride - xyz_col
    if capacity is None:
        capacity = min(n, batch * max_voxels)
    dev = points.device
    nx, ny, nz = [int(g) for g in grid]
    voxels = torch.empty((capacity, max_points, n_feat), dtype=torch.float32, device=dev) if want_voxels else None
    coords = torch.empty((capacity, 4), dtype=torch.int32, device=dev)
    num = torch.empty((capacity,), dtype=torch.int32, device=dev)
    offs = torch.empty((batch + 1,), dtype=torch.int32, device=dev)
    pf = torch.empty((capacity, 64), dtype=torch.float32, device=dev)
    sf = torch.empty((capacity, 32), dtype=torch.float32, device=dev)
    mem = torch.empty((capacity, 64), dtype=torch.float32, device=dev)
    mask = torch.empty((capacity, max_points, 1), dtype=torch.float32, device=dev) if want_mask else None
    if out is not None:
        spatial, spatial_scale = (o.permute(0, 2, 3, 1) for o in out)
        if spatial.shape != (batch, ny, nx, 128) or spatial_scale.shape != (batch, ny, nx, 32) or not spatial.is_contiguous() \
                or not spatial_scale.is_contiguous():
            raise ValueError("encode_fwd: `out` canvases do not match this call")
    else:
        spatial = torch.empty((batch, ny, nx, 128), dtype=torch.float32, device=dev)
        spatial_scale = torch.empty((batch, ny, nx, 32), dtype=torch.float32, device=dev)
    if bank.shape[1] != 64:
        raise ValueError("encode_fwd is specialised for 64 pillar / 64 memory / 32 scale channels")
    if state is not None and (out is None or state.dtype != torch.uint8 or state.numel() != batch * ny * nx or not state.is_contiguous()):
        raise ValueError("encode_fwd: `state` is the (B*ny*nx,) uint8 occupancy of the `out` canvases")
    lo = [float(torch.tensor(v, dtype=torch.float32)) for v in point_cloud_range[:3]]
    vs = [float(torch.tensor(v, dtype=torch.float32)) for v in voxel_size]
    if workspace.key[0] < batch or workspace.key[1] < n:
        raise ValueError("voxelize workspace too small for this call")
    call("hvpr_encode_fwd_f32", points, n, stride, xyz_col, n_feat, frame_offsets, batch, lo[0], lo[1], lo[2], vs[0], vs[1], vs[2], nx, ny,
         nz, int(max_points), int(max_voxels), int(cap_mode), float(offsets[0]), float(offsets[1]), float(offsets[2]), folded["w0"],
         folded["b0"], folded["w1"], folded["b1"], folded["ws0"], folded["bs0"], folded["ws1"], folded["bs1"], *_bank_args(bank), int(k),
         voxels, coords, num, offs, capacity, pf, sf, mask, mem, spatial, spatial_scale, state, workspace.buf, workspace.buf.numel(),
         workspace.key[0], workspace.key[1], int(index_mode), _stream())
    return {"voxels": voxels, "coords": coords, "num_points": num, "voxel_offsets": offs, "pillar_features": pf,
            "pillar_scale_features": sf, "pillar_mask": mask, "memory_features": mem,
            "spatial": spatial.permute(0, 3, 1, 2), "spatial_scale": spatial_scale.permute(0, 3, 1, 2)}


def canvas_buffers(batch, nx, ny, device):
    """A persistent pair of zeroed canvases + their occupancy state for encode_fwd(out=..., state=...): (spatial (B,128,ny,nx),
    spatial_scale (B,32,ny,nx)) in channels_last memory format and the uint8 state.  Nobody else may write them."""
    sp = torch.zeros((batch, ny, nx, 128), dtype=torch.float32, device=device).permute(0, 3, 1, 2)
    sc = torch.zeros((batch, ny, nx, 32), dtype=torch.float32, device=device).permute(0, 3, 1, 2)
    return (sp, sc), torch.zeros((batch * ny * nx,), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------------ convolutions
class PackedConv:
    """Weights of one conv layer in the kernel's layout [taps, Cin/8, 2, cout_pad, 4] with BatchNorm folded."""

    __slots__ = ("w", "bias", "taps", "stride", "cout", "cout_pad", "up", "cin", "relu", "tile_cfg", "tabs")

    def __init__(self, w, bias, taps, stride, cout, cout_pad, up, cin, relu, tile_cfg):
        self.w, self.bias, self.taps, self.stride = w, bias, taps, stride
        self.cout, self.cout_pad, self.up, self.cin, self.relu, self.tile_cfg = cout, cout_pad, up, cin, relu, tile_cfg
        self.tabs = {}        # walk tables by (N, H, W): _walk_table


def _tile_channels(tile_cfg):
    return 128 if tile_cfg == 0 else 64


def pack_conv(weight, scale=None, shift=None, stride=1, relu=True, tile_cfg=0):
    """weight (Cout, Cin, k, k) with k in {1,3}; scale/shift: folded BatchNorm (per Cout) or None / conv bias."""
    cout, cin, kh, kw = weight.shape
    assert kh == kw and kh in (1, 3) and cin % 8 == 0
    w = weight.detach().float()
    if scale is not None:
        w = w * scale.view(-1, 1, 1, 1)
    tc = _tile_channels(tile_cfg)
    cout_pad = (cout + tc - 1) // tc * tc
    taps = kh * kw
    # (Cout, Cin, kh, kw) -> (taps, Cin/8, 2 halves, Cout, 4)
    p = w.permute(2, 3, 1, 0).reshape(taps, cin // 8, 2, 4, cout).permute(0, 1, 2, 4, 3)
    wp = torch.zeros((taps, cin // 8, 2, cout_pad, 4), dtype=torch.float32, device=w.device)
    wp[:, :, :, :cout] = p
    b = torch.zeros((cout_pad,), dtype=torch.float32, device=w.device)
    if shift is not None:
        b[:cout] = shift.detach().float()
    return PackedConv(wp.contiguous(), b, taps, stride, cout, cout_pad, 1, cin, relu, tile_cfg)


_zero_bias = {}


class PackedConvWino:
    """Stride-1 3x3 conv weights in the Winograd kernel's stage image (hvpr_conv2d_wino_pack_f32) with BatchNorm folded."""

    __slots__ = ("w", "bias", "cout", "cout_pad", "cin", "relu", "px_groups", "tabs")
    taps, stride, up = 9, 1, 1

    def __init__(self, w, bias, cout, cout_pad, cin, relu, px_groups):
        self.w, self.bias, self.cout, self.cout_pad, self.cin, self.relu, self.px_groups = w, bias, cout, cout_pad, cin, relu, px_groups
        self.tabs = {}        # walk tables by (N, H, W): _walk_table


def _walk_table(pc, N, H, W, device):
    """The packed layer's walk table for (N, H, W) — the items of the persistent kernel's walk, read instead of divided for — or
    None (the in-kernel decode).  The table is a tensor on the packed-layer object, built by the first eager call with the
    shape, so it lives as long as the packed weights a captured graph bakes in; a call inside a capture that finds none passes None
    and neither allocates nor launches the builder."""
    key = (N, H, W)
    t = pc.tabs.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        if isinstance(pc, PackedConvWino):
            shape, op = (N, H, W, pc.cout, pc.px_groups), "hvpr_conv2d_wino_tab"
        else:
            shape, op = (N, H, W, pc.taps, pc.stride, pc.cout_pad, pc.tile_cfg), "hvpr_conv2d_tab"
        nbytes = getattr(lib(), op + "_bytes")(*shape)
        t = torch.empty((nbytes // 8,), dtype=torch.int64, device=device)
        if nbytes:
            call(op + "_build", *shape, t, _stream())
            torch.cuda.current_stream().synchronize()      # once per layer and shape: later calls may come on any stream
        pc.tabs[key] = t
    return t if t.numel() else None


def pack_conv_wino(weight, scale=None, shift=None, relu=True, px_groups=1, adjoint=False):
    """weight (Cout, Cin, 3, 3) [adjoint: (Cin, Cout, 3, 3) of the layer whose data gradient is wanted]; scale / shift as in
    pack_conv.  Packs on the device (one small kernel), so the training step can repack every call."""
    w = weight.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    cout, cin = (w.shape[1], w.shape[0]) if adjoint else (w.shape[0], w.shape[1])
    assert w.shape[2:] == (3, 3) and cin % 8 == 0 and cout % 4 == 0
    cout_pad = (cout + 63) // 64 * 64
    wp = torch.empty((lib().hvpr_conv2d_wino_packed_floats(cin, cout),), dtype=torch.float32, device=w.device)
    sc = None if scale is None else scale.detach().float().contiguous()
    call("hvpr_conv2d_wino_pack_f32", w, sc, cout, cin, 1 if adjoint else 0, wp, _stream())
    if shift is None:                     # raw convolutions (training: packed every call) share one zero bias per size
        key = (cout_pad, w.device)
        if key not in _zero_bias:
            _zero_bias[key] = torch.zeros((cout_pad,), dtype=torch.float32, device=w.device)
        b = _zero_bias[key]
    else:
        b = torch.zeros((cout_pad,), dtype=torch.float32, device=w.device)
        b[:cout] = shift.detach().float()
    return PackedConvWino(wp, b, cout, cout_pad, cin, relu, px_groups)


def conv2d_wino_nhwc(x, pc, out=None, out_coff=0, gate=None, resid=None, bn_partials=None, use_table=False):
    """x (N,H,W,Cin) contiguous f32 -> (N,H,W,C): 3x3 / stride 1 / pad 1 by Winograd F(2x2,3x3); arguments as conv2d_nhwc.
    use_table: read the walk's items from the layer's table (_walk_table) where the kernel takes one — for layers that are packed
    once and called many times (eval); False: the in-kernel decode.
    bn_partials: (hvpr_conv2d_wino_stats_rows(N,H,W), 2, C) f32 to receive the per-tile sums of the raw output (training)."""
    N, H, W, cin = x.shape
    assert cin == pc.cin
    if out is None:
        out = torch.empty((N, H, W, pc.cout), dtype=torch.float32, device=x.device)
    assert out.shape[:3] == (N, H, W) and out.is_contiguous()
    tab = _walk_table(pc, N, H, W, x.device) if use_table and bn_partials is None and pc.px_groups == 1 else None
    call("hvpr_conv2d_wino_nhwc_tab_f32", x, N, H, W, cin, pc.w, pc.bias, pc.cout, 1 if pc.relu else 0, gate, resid,
         0 if resid is None else resid.shape[-1], out, out.shape[-1], int(out_coff), pc.px_groups, bn_partials, tab, _stream())
    return out


def pack_deconv(weight, scale, shift, relu=True, tile_cfg=0):
    """ConvTranspose2d weight (Cin, Cout, s, s) with kernel == stride == s -> 1x1 GEMM with s*s*Cout columns."""
    cin, cout, s, s2 = weight.shape
    assert s == s2 and cin % 8 == 0
    w = weight.detach().float() * scale.view(1, -1, 1, 1)
    cols = s * s * cout
    tc = _tile_channels(tile_cfg)
    cout_pad = (cols + tc - 1) // tc * tc
    # column = (ky*s + kx)*Cout + co
    g = w.permute(0, 2, 3, 1).reshape(cin, cols)                       # (Cin, cols)
    p = g.reshape(cin // 8, 2, 4, cols).permute(0, 1, 3, 2).unsqueeze(0)     # (1, Cin/8, 2, cols, 4)
    wp = torch.zeros((1, cin // 8, 2, cout_pad, 4), dtype=torch.float32, device=w.device)
    wp[:, :, :, :cols] = p
    b = torch.zeros((cout_pad,), dtype=torch.float32, device=w.device)
    b[:cols] = shift.detach().float().repeat(s * s)
    return PackedConv(wp.contiguous(), b, 1, 1, cout, cout_pad, s, cin, relu, tile_cfg)


def conv_algo():
    """Algorithm of the stride-1 3x3 convolutions: "winograd" (hvpr_conv2d_wino_nhwc_f32, default) or "direct"
    (hvpr_conv2d_nhwc_f32; HVPR_CONV_ALGO=direct).  Every other shape always takes the direct kernel."""
    algo = os.environ.get("HVPR_CONV_ALGO", "winograd")
    if algo not in ("winograd", "direct"):
        raise ValueError(f"HVPR_CONV_ALGO must be 'winograd' or 'direct', got {algo!r}")
    return algo


def pack_conv_auto(weight, scale=None, shift=None, stride=1, relu=True, tile_cfg=1, px_groups=1):
    """pack_conv_wino for a 3x3 / stride-1 layer when conv_algo() is "winograd", pack_conv otherwise; conv2d_nhwc takes either."""
    if weight.shape[2] == 3 and stride == 1 and weight.shape[0] % 4 == 0 and weight.shape[1] % 8 == 0 and conv_algo() == "winograd":
        return pack_conv_wino(weight, scale, shift, relu=relu, px_groups=px_groups)
    return pack_conv(weight, scale, shift, stride=stride, relu=relu, tile_cfg=tile_cfg)


def conv2d_nhwc(x, pc, out=None, out_coff=0, gate=None, resid=None, use_table=False):
    """x (N,H,W,Cin) contiguous f32 -> (N,OH*up,OW*up,C) ; optional fused y = gate*y + resid (SFM step).  The packed type selects the
    kernel.  A PackedConvBf3 takes split-bf16 activations (split_bf16) and returns them, or fp32 when pc.out_split is off or it is
    a deconvolution; split-bf16 activations handed to an fp32 layer are recombined first."""
    if isinstance(pc, PackedConvBf3):
        if pc.up is not None:
            assert gate is None and resid is None
            return deconv_nhwc_bf3(x, pc, out, out_coff=out_coff)
        assert out is None, "the split-bf16 convolution allocates its own output"
        return conv2d_nhwc_bf3(x, pc, out_split=pc.out_split, gate=gate, resid=resid)
    if x.dtype == torch.bfloat16:
        x = unsplit_bf16(x)
    if isinstance(pc, PackedConvWino):
        return conv2d_wino_nhwc(x, pc, out=out, out_coff=out_coff, gate=gate, resid=resid, use_table=use_table)
    N, H, W, cin = x.shape
    assert cin == pc.cin
    if pc.taps == 9:
        OH, OW = (H + 2 - 3) // pc.stride + 1, (W + 2 - 3) // pc.stride + 1
    else:
        OH, OW = H, W
    if out is None:
        out = torch.empty((N, OH * pc.up, OW * pc.up, pc.cout), dtype=torch.float32, device=x.device)
    assert out.shape[:3] == (N, OH * pc.up, OW * pc.up) and out.is_contiguous()
    tab = _walk_table(pc, N, H, W, x.device) if use_table else None
    call("hvpr_conv2d_nhwc_tab_f32", x, N, H, W, cin, pc.w, pc.bias, pc.taps, pc.stride, pc.cout, pc.cout_pad, pc.up, 1 if pc.relu else 0,
         gate, resid, 0 if resid is None else resid.shape[-1], out, out.shape[-1], int(out_coff), pc.tile_cfg, tab, _stream())
    return out


def pack_conv_s2_dgrad(weight):
    """The weight image conv2d_s2_dgrad_nhwc multiplies with: the filter with its channel axes swapped, taps not flipped."""
    return pack_conv(weight.detach().permute(1, 0, 2, 3), None, None, stride=1, relu=False, tile_cfg=1)


def conv2d_s2_dgrad_nhwc(dz, weight, H, W, pc=None):
    """Data gradient of a 3x3 stride-2 (pad 1) convolution with `weight` (Cout, Cin, 3, 3): dz (N,OH,OW,Cout) -> dx (N,H,W,Cin), gathered
    per output-pixel parity class (hvpr_conv2d_s2_dgrad_nhwc_f32: 2.25 taps per pixel instead of a stride-1 convolution's 9 over a
    zero-upsampled dz)."""
    N, OH, OW, cout = dz.shape
    cin = weight.shape[1]
    assert weight.shape[0] == cout and tuple(weight.shape[2:]) == (3, 3) and OH == (H + 2 - 3) // 2 + 1 and OW == (W + 2 - 3) // 2 + 1
    if pc is None:
        pc = pack_conv_s2_dgrad(weight)                                                                    # (Cin, Cout, 3, 3): taps not flipped
    dx = torch.empty((N, H, W, cin), dtype=torch.float32, device=dz.device)
    call("hvpr_conv2d_s2_dgrad_nhwc_f32", dz, N, OH, OW, cout, pc.w, pc.bias, cin, pc.cout_pad, H, W, dx, cin, 0, _stream())
    return dx


# ------------------------------------------------------------------------------------------------ gate / decode / top-k / NMS
def spatial_gate(y_nhwc, w18, conv_bias, bn_scale, bn_shift):
    N, H, W, C = y_nhwc.shape
    gate = torch.empty((N, H, W), dtype=torch.float32, device=y_nhwc.device)
    call("hvpr_spatial_gate_f32", y_nhwc, N, H, W, C, w18, float(conv_bias), float(bn_scale), float(bn_shift), gate, _stream())
    return gate


def head_decode(head_nhwc, n_anchor, n_class, n_dir_bins, x_shifts, y_shifts, anchor_table, dir_offset, dir_limit_offset,
                period, want_cls=True, want_scores=True, out=None):
    N, H, W, CH = head_nhwc.shape
    A = H * W * n_anchor
    dev = head_nhwc.device
    if out is not None:      # (cls, box, scores, labels) of an earlier call with the same shapes
        cls, box, scores, labels = out
        if box.shape != (N, A, 7) or not all(t is None or t.is_contiguous() for t in out):
            raise ValueError("head_decode: `out` tensors do not match this call")
    else:
        cls = torch.empty((N, A, n_class), dtype=torch.float32, device=dev) if want_cls else None
        box = torch.empty((N, A, 7), dtype=torch.float32, device=dev)
        scores = torch.empty((N, A), dtype=torch.float32, device=dev) if want_scores else None
        labels = torch.empty((N, A), dtype=torch.int32, device=dev) if want_scores else None
    call("hvpr_head_decode_f32", head_nhwc, N, H, W, CH, n_anchor, n_class, n_dir_bins, x_shifts, y_shifts, anchor_table, float(dir_offset),
         float(dir_limit_offset), float(period), cls, box, scores, labels, _stream())
    return cls, box, scores, labels


# Most segments (frames, or frame x class lists) one batched NMS call takes.  A segment's workspace is about 19.5 MB at
# pre_max = 4096 (2 MB of mask, 17 MB of per-tile pair segments, the prepared boxes), so 16 segments are 312 MB and the 48 of
# 16 frames x 3 classes would be 0.93 GB: callers walk longer batches in chunks of this many through one workspace.
MAX_NMS_SEGMENTS = 16


class PostWorkspace:
    """Device scratch for score top-k + NMS of `batch` score rows with `n_scores` anchors each.  `segments` (default: `batch`) is the
    number of candidate lists a batched NMS call will be given; `.nms` holds min(segments, MAX_NMS_SEGMENTS) of them
    (`.nms_segments`): hvpr_nms_bev_batched_workspace_bytes(segments, pre_max) bytes, about 19.5 MB per segment at pre_max = 4096,
    312 MB at the cap of 16.  It serves kernels.nms_bev (one list) as well."""

    def __init__(self, batch, n_scores, pre_max, device, segments=None):
        self.batch, self.n_scores, self.pre_max = batch, n_scores, pre_max
        self.nms_segments = max(1, min(batch if segments is None else int(segments), MAX_NMS_SEGMENTS))
        # zero-filled once: every hvpr_score_topk_f32 call leaves its counters and histogram zeroed again
        self.topk = torch.zeros(lib().hvpr_score_topk_workspace_bytes(batch, n_scores), dtype=torch.uint8, device=device)
        self.nms = torch.empty(lib().hvpr_nms_bev_batched_workspace_bytes(self.nms_segments, pre_max), dtype=torch.uint8, device=device)


def score_topk(scores, score_thresh, pre_max, ws, want_scores=True):
    """scores (B, A) -> order (B, pre_max) i32, sorted scores (B, pre_max), counts (B,) i32."""
    B, A = scores.shape
    if B != ws.batch:     # the workspace's zero state is laid out per frame
        raise ValueError(f"score_topk: {B} frames on a workspace made for {ws.batch}")
    dev = scores.device
    order = torch.empty((B, pre_max), dtype=torch.int32, device=dev)
    ss = torch.empty((B, pre_max), dtype=torch.float32, device=dev) if want_scores else None
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    use = score_thresh is not None
    call("hvpr_score_topk_f32", scores, B, A, float(score_thresh) if use else 0.0, 1 if use else 0, int(pre_max), order, ss, counts,
         ws.topk, ws.topk.numel(), _stream())
    return order, ss, counts


def nms_bev(boxes, order, n_device, n_max, thresh, max_keep, ws_nms, map_through_order=True):
    """boxes (R, >=7) f32; order (n_max,) i32 or None.  Returns keep (max_keep,) i32, keep_count (1,) i32."""
    dev = boxes.device
    keep = torch.zeros((max(max_keep, 1),), dtype=torch.int32, device=dev)   # rows past keep_count stay valid ids
    kc = torch.empty((1,), dtype=torch.int32, device=dev)
    call("hvpr_nms_bev_f32", boxes, boxes.shape[1], order, n_device, int(n_max), float(thresh), int(max_keep),
         1 if map_through_order else 0, keep, kc, ws_nms, ws_nms.numel(), _stream())
    return keep, kc


def gather_predictions(boxes, scores, labels, keep):
    """boxes (A,>=7), scores (A,), labels (A,) i32, keep (K,) i32 -> pred_boxes (K,7), pred_scores (K,), pred_labels (K,) i64,
    selected (K,) i64 in one launch."""
    K = keep.shape[0]
    dev = boxes.device
    ob = torch.empty((K, 7), dtype=torch.float32, device=dev)
    os_ = torch.empty((K,), dtype=torch.float32, device=dev)
    ol = torch.empty((K,), dtype=torch.int64, device=dev)
    osel = torch.empty((K,), dtype=torch.int64, device=dev)
    call("hvpr_gather_predictions_f32", boxes, boxes.shape[1], scores, labels, keep, K, ob, os_, ol, osel, _stream())
    return ob, os_, ol, osel


def nms_segment_chunks(n_tables, segments_per_table=1):
    """The calls that walk n_tables * segments_per_table candidate lists with at most MAX_NMS_SEGMENTS per call: yields (first
    list, end list, first table, end table, segments_per_table of the call).  Whole tables per call; a table with more lists than
    the cap is walked on its own, a run of its lists at a time."""
    cap, spt = max(int(MAX_NMS_SEGMENTS), 1), int(segments_per_table)
    if spt <= cap:
        step = cap // spt
        for t0 in range(0, n_tables, step):
            t1 = min(n_tables, t0 + step)
            yield t0 * spt, t1 * spt, t0, t1, spt
    else:
        for t in range(n_tables):
            for k0 in range(0, spt, cap):
                k1 = min(spt, k0 + cap)
                yield t * spt + k0, t * spt + k1, t, t + 1, k1 - k0


def nms_call_segments(n_tables, segments_per_table=1):
    """Lists in the largest call of nms_segment_chunks: what a PostWorkspace for them is sized for (`segments=`)."""
    return max((s1 - s0 for s0, s1, _, _, _ in nms_segment_chunks(n_tables, segments_per_table)), default=1)


def nms_bev_batched(boxes, order, n_device, n_max, thresh, max_keep, ws_nms, map_through_order=True, segments_per_table=1):
    """Rotated NMS of S candidate lists in one call (hvpr_nms_bev_batched_f32): boxes (T, R, >=7) f32, T box tables; order
    (S, n_max) i32 or None; n_device (S,) i32 or None (every list holds n_max); list s ranks table s // segments_per_table, so
    S = T * segments_per_table.  Returns keep (S, max_keep) i32, zero-initialised like the single form's, and keep_count (S,) i32:
    per list what nms_bev gives for it alone.  ws_nms holds hvpr_nms_bev_batched_workspace_bytes(S, n_max) bytes (about 19.5 MB
    per list at n_max = 4096; PostWorkspace(...).nms); callers keep S <= MAX_NMS_SEGMENTS and walk longer batches in chunks."""
    if boxes.dim() != 3:
        raise ValueError("nms_bev_batched: boxes must be (tables, rows, >= 7)")
    S = boxes.shape[0] * int(segments_per_table)
    if order is not None and tuple(order.shape) != (S, n_max):
        raise ValueError(f"nms_bev_batched: order must be ({S}, {n_max}), got {tuple(order.shape)}")
    if n_device is not None and tuple(n_device.shape) != (S,):
        raise ValueError(f"nms_bev_batched: n_device must be ({S},), got {tuple(n_device.shape)}")
    dev = boxes.device
    keep = torch.zeros((S, max(max_keep, 1)), dtype=torch.int32, device=dev)   # rows past keep_count stay valid ids
    kc = torch.empty((S,), dtype=torch.int32, device=dev)
    call("hvpr_nms_bev_batched_f32", boxes, boxes.shape[2], boxes.shape[1] * boxes.shape[2], int(segments_per_table), order, n_device, S,
         int(n_max), float(thresh), int(max_keep), 1 if map_through_order else 0, keep, kc, ws_nms, ws_nms.numel(), _stream())
    return keep, kc


def gather_predictions_batched(boxes, scores, labels, keep, segments_per_table=1):
    """boxes (T, A, >=7), scores (S, A), labels (S, A) i32, keep (S, K) i32 -> pred_boxes (S, K, 7), pred_scores (S, K), pred_labels
    (S, K) i64, selected (S, K) i64 in one launch; list s reads table s // segments_per_table."""
    S, K = keep.shape
    if boxes.dim() != 3 or boxes.shape[0] * int(segments_per_table) != S or tuple(scores.shape) != (S, boxes.shape[1]) \
            or labels.shape != scores.shape:
        raise ValueError("gather_predictions_batched: shapes do not match")
    dev = boxes.device
    ob = torch.empty((S, K, 7), dtype=torch.float32, device=dev)
    os_ = torch.empty((S, K), dtype=torch.float32, device=dev)
    ol = torch.empty((S, K), dtype=torch.int64, device=dev)
    osel = torch.empty((S, K), dtype=torch.int64, device=dev)
    call("hvpr_gather_predictions_batched_f32", boxes, boxes.shape[2], boxes.shape[1] * boxes.shape[2], int(segments_per_table), scores,
         labels, scores.shape[1], keep, S, K, ob, os_, ol, osel, _stream())
    return ob, os_, ol, osel


def gather_predictions_multiclass(boxes, scores, keep, keep_count, num_class):
    """The MULTI_CLASSES_NMS records of a batch in one launch, nothing read back: boxes (B, A, >=7), scores (B * nc, A) class-major,
    keep (B * nc, K) i32 and keep_count (B * nc,) i32 as the batched NMS leaves them -> pred_boxes (B, nc * K, 7), pred_scores,
    pred_labels i64 (class + 1), selected i64 (B, nc * K) and pred_count (B,) i32.  A frame's rows are its classes' kept candidates
    in class order; the rows past pred_count hold anchor 0 of class 0."""
    nc = int(num_class)
    S, K = keep.shape
    if boxes.dim() != 3 or nc < 1 or boxes.shape[0] * nc != S or tuple(scores.shape) != (S, boxes.shape[1]) \
            or tuple(keep_count.shape) != (S,):
        raise ValueError("gather_predictions_multiclass: shapes do not match")
    B, dev = boxes.shape[0], boxes.device
    ob = torch.empty((B, nc * K, 7), dtype=torch.float32, device=dev)
    os_ = torch.empty((B, nc * K), dtype=torch.float32, device=dev)
    ol = torch.empty((B, nc * K), dtype=torch.int64, device=dev)
    osel = torch.empty((B, nc * K), dtype=torch.int64, device=dev)
    oc = torch.empty((B,), dtype=torch.int32, device=dev)
    call("hvpr_gather_predictions_multiclass_f32", boxes, boxes.shape[2], boxes.shape[1] * boxes.shape[2], scores, scores.shape[1], keep,
         keep_count, B, nc, K, ob, os_, ol, osel, oc, _stream())
    return ob, os_, ol, osel, oc


def boxes_pairwise(a, b, mode):
    """mode 0: BEV overlap area, 1: BEV IoU, 2: 3D IoU.  a (N,7), b (M,7) -> (N,M)."""
    a = a[:, :7].contiguous()
    b = b[:, :7].contiguous()
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    call("hvpr_boxes_pairwise_f32", a, a.shape[0], b, b.shape[0], int(mode), out, _stream())
    return out


# ------------------------------------------------------------------------------------------------ KITTI AP (f3)
def boxes_pairwise_ragged(a, b, a_off, b_off, pair_off, n_pairs):
    """BEV overlap areas (mode 0) of F independent frames in one launch.  a (NA,7), b (NB,7) f32; a_off, b_off, pair_off (F+1,)
    int64 cuda -> (n_pairs,) f32, frame f at pair_off[f] as its (n_f, m_f) matrix, bit-equal to boxes_pairwise on that frame."""
    out = torch.empty((int(n_pairs),), dtype=torch.float32, device=pair_off.device)
    call("hvpr_boxes_pairwise_ragged_f32", a, b, a_off, b_off, pair_off, pair_off.numel() - 1, int(n_pairs), out, _stream())
    return out


def kitti_overlaps(gt_rows, dt_rows, inter, gt_off, dt_off, pair_off, n_pairs, metric):
    """The host's frame_overlap for every frame: (n_pairs,) f64, frame f at pair_off[f] as its (nd_f, ng_f) matrix."""
    out = torch.empty((int(n_pairs),), dtype=torch.float64, device=pair_off.device)
    call("hvpr_kitti_overlaps_f64", gt_rows, dt_rows, inter, gt_off, dt_off, pair_off, pair_off.numel() - 1, int(n_pairs), int(metric), out,
         _stream())
    return out


def kitti_match(gt_rows, gt_cls, gt_dontcare, dt_rows, dt_cls, gt_off, dt_off, pair_off, overlaps, metric, classes, min_overlaps,
                thresholds=None, thresh_count=None, compute_aos=False, out=None):
    """Greedy matching of every (frame, class, difficulty, overlap set).  classes: class ids; min_overlaps [n_sets, n_classes]
    (host).  Without thresholds, the threshold pass -> (tp_score [combos, NG] f64, n_valid [n_classes, 3] i32); with thresholds
    [combos, T] f64 and thresh_count [combos] i32 (cuda), the counting pass -> (counts [combos, T, 3] i32, sim [combos, T] f64).
    `out`: the pair of tensors to fill instead of new ones."""
    dev = pair_off.device
    F, NG = pair_off.numel() - 1, gt_rows.shape[0]
    C, K = len(classes), len(min_overlaps)
    combos = C * 3 * K
    c_classes = (ctypes.c_int32 * C)(*[int(c) for c in classes])
    c_mo = (ctypes.c_double * (K * C))(*[float(v) for row in min_overlaps for v in row])
    if thresholds is None:
        a, b = out if out is not None else (torch.empty((combos, NG), dtype=torch.float64, device=dev),
                                            torch.empty((C, 3), dtype=torch.int32, device=dev))
        args = (None, None, 1, 0, a, b, None, None, None, 0)
    else:
        T = thresholds.shape[1]
        a, b = out if out is not None else (torch.empty((combos, T, 3), dtype=torch.int32, device=dev),
                                            torch.empty((combos, T), dtype=torch.float64, device=dev))
        ws = torch.empty((lib().hvpr_kitti_match_workspace_bytes(F, C, K, T),), dtype=torch.uint8, device=dev)
        args = (thresholds, thresh_count, T, int(bool(compute_aos)), None, None, a, b, ws, ws.numel())
    call("hvpr_kitti_match_f64", gt_rows, gt_cls, gt_dontcare, dt_rows, dt_cls, gt_off, dt_off, pair_off, F, NG, overlaps, int(metric),
         0 if thresholds is None else 1, c_classes, C, c_mo, K, *args, _stream())
    return a, b


# ------------------------------------------------------------------------------------------------ f5: evaluation epilogue
def recall_record(pred_boxes, pred_count, gt_boxes, thresholds, counts=None, best_iou=None):
    """generate_recall_record for every frame of a batch, no host read.  pred_boxes (B, P, 7) f32 with pred_count (B,) i32 live
    rows; gt_boxes (B, G, C >= 7) f32; thresholds: at most 8 host floats.  -> counts (B, 1 + T) i32 = ground truths, then the
    recalled ones per threshold.  best_iou: an optional (B, G) f32 tensor to fill."""
    B, P = int(pred_boxes.shape[0]), int(pred_boxes.shape[1])
    if pred_boxes.dim() != 3 or pred_boxes.shape[2] != 7 or gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or pred_count.numel() != B:
        raise ValueError("recall_record: pred_boxes (B, P, 7), pred_count (B,) and gt_boxes (B, G, C) must agree")
    G, C, T = int(gt_boxes.shape[1]), int(gt_boxes.shape[2]), len(thresholds)
    if counts is None:
        counts = torch.empty((B, 1 + T), dtype=torch.int32, device=pred_boxes.device)
    if tuple(counts.shape) != (B, 1 + T) or (best_iou is not None and tuple(best_iou.shape) != (B, G)):
        raise ValueError("recall_record: counts must be (B, 1 + T) and best_iou (B, G)")
    thr = (ctypes.c_float * max(T, 1))(*[float(t) for t in thresholds])
    call("hvpr_recall_record_f32", pred_boxes, pred_count, B, P, gt_boxes, G, C, thr, T, counts, best_iou, _stream())
    return counts


def prediction_annos(pred_boxes, pred_scores, pred_labels, pred_count, calib, class_of_label, row_base, frame_base, dt_rows, dt_cls,
                     dt_label, dt_box7, boxes_lidar, dt_off, overflow):
    """generate_prediction_dicts for a batch into the caller's split-wide tables, no host read: frame b's live rows follow frame
    b - 1's from row_base[0] (a device int64 word, advanced here) on; dt_off[frame_base + b + 1] is set.  calib (B, 26) f32 cuda
    (calibration.pack_calib), class_of_label: host ints, label - 1 -> evaluator class id."""
    B, P = int(pred_boxes.shape[0]), int(pred_boxes.shape[1])
    if tuple(pred_boxes.shape) != (B, P, 7) or tuple(pred_scores.shape) != (B, P) or tuple(pred_labels.shape) != (B, P) \
            or pred_count.numel() != B or tuple(calib.shape) != (B, 26):
        raise ValueError("prediction_annos: shapes do not match")
    cap = int(dt_rows.shape[0])
    if tuple(dt_rows.shape) != (cap, 16) or dt_cls.numel() != cap or dt_label.numel() != cap or tuple(dt_box7.shape) != (cap, 7) \
            or tuple(boxes_lidar.shape) != (cap, 7):
        raise ValueError("prediction_annos: the tables must hold the same number of rows")
    n = len(class_of_label)
    cmap = (ctypes.c_int32 * max(n, 1))(*[int(c) for c in class_of_label])
    call("hvpr_prediction_annos_f32", pred_boxes, pred_scores, pred_labels, pred_count, B, P, calib, cmap, n, row_base, cap,
         int(frame_base), dt_off.numel() - 1, dt_rows, dt_cls, dt_label, dt_box7, boxes_lidar, dt_off, overflow, _stream())


# ------------------------------------------------------------------------------------------------ f4: training augmentation
def augment_block_points():
    """Scene points per workgroup of the point passes."""
    return int(lib().hvpr_augment_block_points())


def augment_collide(plan_host, plan_dev, words):
    """valid (C,) int32: which candidates of the packed plan may be pasted.  `plan_host` is the (pinned) int32 host tensor the
    device copy `plan_dev` was made from; the library checks it before it launches anything."""
    C = int(plan_host.numpy()[4])
    valid = torch.zeros((max(C, 1),), dtype=torch.int32, device=plan_dev.device)
    # the *_host tensors live in host memory: raw addresses
    call("hvpr_augment_collide_f32", plan_host.data_ptr(), plan_dev, int(words), valid, _stream())
    return valid[:C]


def augment_boxes(plan_host, plan_dev, words, valid, point_cloud_range, remove_outside, g_cap, out=None, count=None):
    """(gt_boxes (B, g_cap, 8), count (B,) int32)."""
    B = int(plan_host.numpy()[1])
    rng6 = np.ascontiguousarray(point_cloud_range, np.float32)
    if out is None:
        out = torch.empty((B, g_cap, 8), dtype=torch.float32, device=plan_dev.device)
    if count is None:
        count = torch.empty((B,), dtype=torch.int32, device=plan_dev.device)
    # the *_host tensors live in host memory: raw addresses
    call("hvpr_augment_boxes_f32", plan_host.data_ptr(), plan_dev, int(words), valid, rng6.ctypes.data, int(bool(remove_outside)),
         int(g_cap), out, count, _stream())
    return out, count


def augment_points(plan_host, plan_dev, words, valid, points, bank_points, bank_boxes, extra_width, out=None, out_off=None):
    """(out_points (capacity, F), out_off (B+1,) int32).  capacity = scene points + the points of all candidates, known on the
    host: nothing is read to allocate."""
    h = plan_host.numpy()                      # the host copy: header B, NG, G, C; pt_off and cand_n as csrc/augment.hip lays them out
    B, NG, G, C = int(h[1]), int(h[2]), int(h[3]), int(h[4])
    n, F = points.shape
    ex = np.ascontiguousarray(extra_width, np.float32)
    pt_off = h[8 + (B + 1) + (B * NG + 1):][: B + 1]
    max_frame = int(np.diff(pt_off).max()) if B > 0 else 0
    if out is None:
        c5 = 8 + (B + 1) + (B * NG + 1) + (B + 1) + G + 4 * C
        out = torch.empty((n + int(h[c5: c5 + C].sum()), F), dtype=torch.float32, device=points.device)
    if out_off is None:
        out_off = torch.empty((B + 1,), dtype=torch.int32, device=points.device)
    ws = _workspace(None, lib().hvpr_augment_points_workspace_bytes(B, max_frame, C, n), points.device)
    # the *_host tensors live in host memory: raw addresses
    call("hvpr_augment_points_f32", plan_host.data_ptr(), plan_dev, int(words), valid, points, n, F, bank_points, bank_points.shape[0],
         bank_boxes, bank_boxes.shape[0], bank_points.shape[1], ex.ctypes.data, out, out.shape[0], out_off, ws, ws.numel(), _stream())
    return out, out_off


def augment_batch(plan_host, plan_dev, words, points, bank, extra_width, point_cloud_range, remove_outside, g_cap):
    """All launches of one DeviceAugmentor call.  `counts` (2B+1,) int32 holds the point offsets, then the box counts: the one
    buffer the caller reads."""
    B = int(plan_host.numpy()[1])
    arena, obj_box = bank.on_device()
    counts = torch.empty((2 * B + 1,), dtype=torch.int32, device=points.device)
    valid = augment_collide(plan_host, plan_dev, words)
    gt, _ = augment_boxes(plan_host, plan_dev, words, valid, point_cloud_range, remove_outside, g_cap, count=counts[B + 1:])
    pts, off = augment_points(plan_host, plan_dev, words, valid, points, arena, obj_box, extra_width, out_off=counts[: B + 1])
    return {"points": pts, "point_frame_offsets": off, "gt_boxes": gt, "valid": valid, "counts": counts}


# ------------------------------------------------------------------------------------------------ f6: the GT-sampling database
def gt_database_block_points():
    """Scene points per workgroup of the count and write passes."""
    return int(lib().hvpr_gt_database_block_points())


def _chunk_count_prologue(pt_off_host, n_obj, device, obj_count, workspace, workspace_bytes):
    """(obj_count, workspace) as both count calls of a staged chunk begin: the largest frame from the host offsets, the workspace
    `workspace_bytes(B, largest frame, n_obj)` asks for, and `obj_count` (n_obj,) int32 where none is given."""
    off = pt_off_host.numpy()
    max_frame = int(np.diff(off).max()) if off.shape[0] > 1 else 0
    if obj_count is None:
        obj_count = torch.empty((max(n_obj, 1),), dtype=torch.int32, device=device)[:n_obj]
    return obj_count, _workspace(workspace, workspace_bytes(off.shape[0] - 1, max_frame, n_obj), device)


def gt_database_count(points, pt_off_host, pt_off, boxes, box_off_host, box_off, obj_count=None, workspace=None):
    """(obj_count (n_obj,) int32, workspace).  points (sum N, F) and boxes (n_obj, 7) float32 on the device; `pt_off_host` /
    `box_off_host` are the int32 host tensors (B + 1,) the device copies `pt_off` / `box_off` were made from: the library checks
    them before it launches anything.  The workspace goes to gt_database_extract of the same chunk."""
    n, F = points.shape
    n_obj, B = int(boxes.shape[0]), pt_off_host.numel() - 1
    obj_count, workspace = _chunk_count_prologue(pt_off_host, n_obj, points.device, obj_count, workspace,
                                                 lib().hvpr_gt_database_workspace_bytes)
    # the *_host tensors live in host memory: raw addresses
    call("hvpr_gt_database_count_f32", points, n, F, pt_off_host.data_ptr(), pt_off, B, boxes, box_off_host.data_ptr(), box_off, n_obj,
         obj_count, workspace, workspace.numel(), _stream())
    return obj_count, workspace


def gt_database_extract(points, pt_off_host, pt_off, boxes, box_off_host, box_off, centres, obj_count_host, obj_count, arena,
                        workspace, obj_off=None):
    """obj_off (n_obj + 1,) int32; writes `arena` (capacity, F) rows obj_off[k] .. obj_off[k + 1] for every box k.  `workspace`
    is the one gt_database_count filled for this chunk, `obj_count_host` the int32 host tensor of the counts read back."""
    n, F = points.shape
    n_obj, B = int(boxes.shape[0]), pt_off_host.numel() - 1
    if arena.shape[1] != F:
        raise ValueError("gt_database_extract: the arena must have the points' feature width")
    if obj_off is None:
        obj_off = torch.empty((n_obj + 1,), dtype=torch.int32, device=points.device)
    # the *_host tensors live in host memory: raw addresses
    call("hvpr_gt_database_extract_f32", points, n, F, pt_off_host.data_ptr(), pt_off, B, boxes, box_off_host.data_ptr(), box_off, centres,
         n_obj, obj_count_host.data_ptr(), obj_count, obj_off, arena, arena.shape[0], workspace, workspace.numel(), _stream())
    return obj_off


# ------------------------------------------------------------------------------------------------ f8: get_infos' counts
def kitti_infos_block_points():
    """Scene points per workgroup of the count pass (the database's block)."""
    return int(lib().hvpr_kitti_infos_block_points())


def kitti_infos_count(points, pt_off_host, pt_off, boxes, box_off_host, box_off, calib_host, calib, obj_count=None, fov_count=None,
                      want_fov=False, workspace=None):
    """(obj_count (n_obj,) int32, fov_count (B,) int32 or None, workspace): per box the points of its frame in the camera's view
    and inside it, per frame (with `want_fov` or a `fov_count` tensor) the points in view.  The chunk as gt_database_count takes
    it; `calib_host` is the (B, 26) float32 host tensor (calibration.pack_calib) the device copy `calib` was made from.  The library
    checks the host copies before it launches anything."""
    n, F = points.shape
    n_obj, B = int(boxes.shape[0]), pt_off_host.numel() - 1
    if calib_host.dtype != torch.float32 or calib_host.numel() != 26 * B or not calib_host.is_contiguous() or calib_host.is_cuda:
        raise ValueError("kitti_infos_count: calib_host must be a contiguous (B, 26) float32 host tensor")
    if calib.numel() != 26 * B:
        raise ValueError("kitti_infos_count: calib must be (B, 26)")
    if fov_count is None and want_fov:
        fov_count = torch.empty((B,), dtype=torch.int32, device=points.device)
    obj_count, workspace = _chunk_count_prologue(pt_off_host, n_obj, points.device, obj_count, workspace,
                                                 lib().hvpr_kitti_infos_workspace_bytes)
    # the *_host tensors live in host memory: raw addresses
    call("hvpr_kitti_infos_count_f32", points, n, F, pt_off_host.data_ptr(), pt_off, B, boxes, box_off_host.data_ptr(), box_off, n_obj,
         calib_host.data_ptr(), calib, obj_count, fov_count, workspace, workspace.numel(), _stream())
    return obj_count, fov_count, workspace


# ------------------------------------------------------------------------------------------------ f7: ragged select / collate
def ragged_select_tile_rows():
    """Rows per workgroup of the count and write passes."""
    return int(lib().hvpr_ragged_select_tile_rows())


def _workspace(workspace, need, device):
    """`workspace` where it holds `need` bytes, else a new uint8 one of at least 256."""
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(int(need), 256),), dtype=torch.uint8, device=device)
    return workspace


def _ragged_head(points, off, mask, calib, range_xy):
    """(rows, F, B, head, range): `head` is the arguments every hvpr_ragged_* call begins with; `range` owns the host floats
    `head` points to and has to outlive the call."""
    rows, F = points.shape
    B = off.numel() - 1
    r = None if range_xy is None else np.ascontiguousarray(range_xy, np.float32).reshape(4)
    head = (points, rows, F, off, B, int(mask), calib, None if r is None else r.ctypes.data)
    return rows, F, B, head, r


def _offsets(t, B, device):
    return torch.empty((B + 1,), dtype=torch.int32, device=device) if t is None else t


def _out_and_flag(out, flag, rows, width, device):
    if out is None:
        out = torch.empty((rows, width), dtype=torch.float32, device=device)
    if flag is None:
        flag = torch.zeros((1,), dtype=torch.int32, device=device)
    return out, flag


def ragged_select_count(points, off, mask, calib=None, range_xy=None, new_off=None, workspace=None):
    """(new_off (B+1,) int32, workspace).  points (rows, F) float32 and off (B+1,) int32 on the device, `calib` (B, 26) float32
    on the device (calibration.pack_calib) for mask bit 1, `range_xy` four host floats (x0, y0, x1, y1) for mask bit 2.  Rows at or
    past off[B] are ignored.  Nothing is read: the workspace goes to ragged_select_write of the same input."""
    rows, F, B, head, _r = _ragged_head(points, off, mask, calib, range_xy)
    new_off = _offsets(new_off, B, points.device)
    workspace = _workspace(workspace, lib().hvpr_ragged_select_workspace_bytes(rows, B), points.device)
    call("hvpr_ragged_select_count_f32", *head, new_off, workspace, workspace.numel(), _stream())
    return new_off, workspace


def ragged_select_write(points, off, mask, new_off, workspace, calib=None, range_xy=None, inv_perm=None, batch_column=False,
                        out=None, flag=None):
    """(out, flag).  `out` (capacity, F + batch_column) float32: the kept rows, stable, each at its flat rank or, with the flat
    int32 `inv_perm`, at new_off[b] + inv_perm[rank]; `flag` (1,) int32 is set when a row had to be dropped (an inv_perm entry
    outside its frame, an output too small).  Without `out` the output is sized by the input rows: no read is needed."""
    rows, F, B, head, _r = _ragged_head(points, off, mask, calib, range_xy)
    out, flag = _out_and_flag(out, flag, rows, F + (1 if batch_column else 0), points.device)
    call("hvpr_ragged_select_write_f32", *head, new_off, inv_perm, 0 if inv_perm is None else inv_perm.numel(), int(bool(batch_column)),
         out, out.shape[0], flag, workspace, workspace.numel(), _stream())
    return out, flag


def ragged_sample_count(points, off, mask, calib=None, range_xy=None, near=40.0, new_off=None, near_off=None, workspace=None):
    """(new_off, near_off, workspace): ragged_select_count with the second count sample_points needs.  near_off[b] = kept rows in
    front of off[b] with ||xyz|| < near.  Nothing is read: the workspace goes to ragged_sample_write of the same input."""
    rows, F, B, head, _r = _ragged_head(points, off, mask, calib, range_xy)
    new_off, near_off = _offsets(new_off, B, points.device), _offsets(near_off, B, points.device)
    workspace = _workspace(workspace, lib().hvpr_ragged_sample_workspace_bytes(rows, B), points.device)
    call("hvpr_ragged_sample_count_f32", *head, float(near), new_off, near_off, workspace, workspace.numel(), _stream())
    return new_off, near_off, workspace


def ragged_sample_write(points, off, mask, new_off, near_off, mode, dest, num_points, workspace, calib=None, range_xy=None,
                        near=40.0, batch_column=False, out=None, flag=None):
    """(out, flag).  `out` (B * num_points, F + batch_column) float32: every kept row at out[b * num_points + d] for each of its
    two destinations d >= 0 in `dest` (total kept, 2) int32, indexed by new_off[b] + the row's source ordinal: its in-frame rank
    where `mode` (B,) int32 is 0, near ordinals first and far ones behind them where it is 1.  `flag` (1,) int32 is set when a
    store had to be dropped (a destination outside [-1, num_points), a table or an output too small)."""
    rows, F, B, head, _r = _ragged_head(points, off, mask, calib, range_xy)
    out, flag = _out_and_flag(out, flag, B * int(num_points), F + (1 if batch_column else 0), points.device)
    if mode.numel() != B or dest.dim() != 2 or dest.shape[1] != 2:
        raise ValueError("hvpr_amd: mode must be (B,) and dest (n, 2)")
    call("hvpr_ragged_sample_write_f32", *head, float(near), new_off, near_off, mode, dest, dest.shape[0], int(num_points),
         int(bool(batch_column)), out, out.shape[0], flag, workspace, workspace.numel(), _stream())
    return out, flag


# ------------------------------------------------------------------------------------------------ v1: the BEV picture
def bev_grid(point_cloud_range, pixel):
    """(H, W) of the picture: round((hi - lo) / pixel) in float32, y cells by x cells (tools/vis.py:90-91)."""
    r = np.ascontiguousarray(point_cloud_range, np.float32).reshape(6)
    g = np.round((r[3:5] - r[:2]) / np.float32(pixel)).astype(np.int64)
    return int(g[1]), int(g[0])


def render_bev(points, frame_offsets, point_cloud_range, pixel, palette, tables=(), xyz_col=0, thickness=2, heading_sign=-1,
               image=None, counts=None, want_counts=False, workspace=None):
    """(image (B, H, W, 3) uint8, counts (B, H, W) int32 or None, workspace): the height picture of the ragged `points`
    (n, stride) float32 with `frame_offsets` (B + 1,) int32 on the device, and on it the outlines of up to two box tables.  A
    table is a dict: `boxes` (B, P, >= 7) float32, optionally `count` (B,) int32, `scores` (B, P) float32 with `thresh`, `labels`
    (B, P) int64, and `ink` (a row's ink is ink + label; ink alone without labels).  `palette` (n_ink, 3) uint8 on the device,
    ink 0 unused.  heading_sign -1 draws a lidar heading as it is, +1 mirrored as the reference does.  Only enqueues."""
    tables = list(tables)
    if len(tables) > 2:
        raise ValueError("render_bev: two box tables at the most")
    if points.dim() != 2 or frame_offsets.dim() != 1 or frame_offsets.numel() < 2:
        raise ValueError("render_bev: points must be (n, stride) and frame_offsets (B + 1,)")
    n, stride = points.shape
    B = frame_offsets.numel() - 1
    rng = np.ascontiguousarray(point_cloud_range, np.float32).reshape(6)
    H, W = bev_grid(rng, pixel)
    need = lib().hvpr_render_bev_workspace_bytes(B, H, W)
    if need == 0:
        raise ValueError(f"render_bev: a picture of {B} x {H} x {W} pixels is not supported")
    dev = points.device
    if palette.dim() != 2 or palette.shape[1] != 3:
        raise ValueError("render_bev: palette must be (n_ink, 3)")
    if image is None:
        image = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    elif tuple(image.shape) != (B, H, W, 3):
        raise ValueError(f"render_bev: image must be {(B, H, W, 3)}")
    if counts is None and want_counts:
        counts = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    elif counts is not None and tuple(counts.shape) != (B, H, W):
        raise ValueError(f"render_bev: counts must be {(B, H, W)}")
    args = []
    for t in tables + [None] * (2 - len(tables)):
        if t is None:
            args += [None, 0, 7, None, None, 0.0, None, 0]
            continue
        boxes = t["boxes"]
        if boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] < 7:
            raise ValueError("render_bev: boxes must be (B, P, >= 7)")
        P = boxes.shape[1]
        for key, shape in (("count", (B,)), ("scores", (B, P)), ("labels", (B, P))):
            if t.get(key) is not None and tuple(t[key].shape) != shape:
                raise ValueError(f"render_bev: {key} must be {shape}")
        args += [boxes if P else None, P, boxes.shape[2], t.get("count"), t.get("scores"), float(t.get("thresh", 0.0)), t.get("labels"),
                 int(t.get("ink", 1))]
    workspace = _workspace(workspace, need, dev)
    call("hvpr_render_bev_u8", points if n else None, n, stride, int(xyz_col), frame_offsets, B, rng.ctypes.data, float(pixel), *args,
         palette, palette.shape[0], int(thickness), int(heading_sign), image, counts, workspace, workspace.numel(), _stream())
    return image, counts, workspace
