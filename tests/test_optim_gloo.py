"""CPU, world_size 2, gloo: FusedSGD inside DistributedDataParallel — what tests/test_distributed_gloo.py does for the flat
Adam-onecycle optimiser, for the flat form of build_optimizer's 'sgd'."""
import os
import socket

import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _flat_sgd_on_cpu(opt):
    """TEST stand-in for the ONE kernel launch of FusedSGD._launch (hvpr_fused_sgd_f32, csrc/train_ops.hip): the same arithmetic
    with torch ops on the flat buffers.  Everything around it — the flat views, zero_grad, the gradient collection under DDP, the
    device-side clip scale — is the product's code and is what this test exercises."""
    g = opt.param_groups[0]
    gs = 1.0 if opt._scale is None else float(opt._scale)
    d = opt.flat_g * gs + g["weight_decay"] * opt.flat_p
    if opt.momentum_buffer is not None:
        opt.momentum_buffer.mul_(g["momentum"]).add_(d)
        d = opt.momentum_buffer
    opt.flat_p.sub_(g["lr"] * d)


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import copy
    import types
    import torch
    torch.set_num_threads(2)
    from hvpr_amd import distributed, optim
    distributed.init("gloo")
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, bias=False), torch.nn.BatchNorm2d(8), torch.nn.ReLU(), torch.nn.Flatten(),
                              torch.nn.Linear(8 * 6 * 6, 4))
    ddp = distributed.wrap_ddp(net, torch.device("cpu"))
    assert isinstance(ddp, torch.nn.parallel.DistributedDataParallel)
    opt = optim.FusedSGD(ddp, lr=0.05, momentum=0.9, weight_decay=0.01)
    opt._launch = types.MethodType(_flat_sgd_on_cpu, opt)
    sched = optim.StepDecayLR(opt, [2], 0.1, 1e-7, 0.05)
    ref = copy.deepcopy(net)                                             # same weights (views into flat_p are deep-copied as tensors)
    ref_opt = torch.optim.SGD(ref.parameters(), lr=0.05, momentum=0.9, weight_decay=0.01)
    ref_sched = optim.StepDecayLR(ref_opt, [2], 0.1, 1e-7, 0.05)
    xs = [[torch.randn(5, 3, 8, 8, generator=torch.Generator().manual_seed(100 * it + r)) for r in range(world)] for it in range(4)]
    ptrs, worst = [], 0.0
    for it in range(4):
        sched.step(it)
        ref_sched.step(it)
        opt.zero_grad()
        ddp(xs[it][rank]).pow(2).mean().backward()
        ptrs.append([p.grad.data_ptr() for p in opt.params])
        opt.clip_grad_norm(0.05)
        opt.step()
        # reference: the rank-mean gradient through torch.optim.SGD
        ref_opt.zero_grad()
        grads = []
        for r in range(world):
            m = copy.deepcopy(ref).train()
            m(xs[it][r]).pow(2).mean().backward()
            grads.append([p.grad for p in m.parameters()])
        ref.train()
        ref(xs[it][rank])                                               # running statistics of this rank's own batch, as DDP keeps them
        for i, p in enumerate(ref.parameters()):
            p.grad = sum(g[i] for g in grads) / world
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.05)
        ref_opt.step()
        for a, b in zip(net.parameters(), ref.parameters()):
            worst = max(worst, float((a.detach() - b.detach()).abs().max() / (b.detach().abs().max() + 1e-12)))
    own = [g.data_ptr() for g in opt._grad_views]
    stable, in_flat = all(p == ptrs[0] for p in ptrs), ptrs[0] == own
    # the ranks' parameters stay equal: every rank sees every other rank's flat buffer
    mine = opt.flat_p.detach().clone()
    both = [torch.zeros_like(mine) for _ in range(world)]
    torch.distributed.all_gather(both, mine)
    same = all(torch.equal(both[0], b) for b in both)
    lrs = (float(opt.lr), ref_opt.param_groups[0]["lr"])
    distributed.finalize()
    q.put((rank, stable, in_flat, same, worst, lrs))


def test_flat_sgd_under_ddp_keeps_grad_addresses_and_the_ranks_equal():
    """Two gloo ranks: p.grad keeps ONE address over the steps and lives in the optimiser's flat buffer, four clipped steps under
    step decay equal torch.optim.SGD on the rank-mean gradients, and both ranks end on the same parameter bits."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    for rank, stable, in_flat, same, worst, lrs in sorted(q.get(timeout=10) for _ in procs):
        assert stable and in_flat and same, (rank, stable, in_flat, same)
        assert worst < 2e-5, (rank, worst)
        assert lrs[0] == lrs[1] == 0.05 * 0.1
