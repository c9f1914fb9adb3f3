"""HIP-graph execution of the step equals eager execution: two trainers with identical seeded weights and identical
(q, beta, noise, batch) run five iterations, one launching every kernel from Python, the other replaying captured
graphs (after its two eager warm-up iterations).  Same kernels, same order, deterministic reductions => the logged
losses and every parameter must agree bit for bit; the skip gate must hold parameters still."""
import pytest
import torch

from tests.golden.seeded_weights import seeded_input
from tests.test_gpu_model import dev
from tests.test_gpu_step import _opt, _seed_params

pytestmark = pytest.mark.gpu


def _trainer(stage, graphs):
    from crdr_amd.trainer import build_trainer
    opt = _opt(stage)
    opt["hip_graphs"] = graphs
    tr = build_trainer(opt)
    _seed_params(tr.comp_model, "")
    if stage == 3:
        _seed_params(tr.discriminator, "")
    _seed_params(tr.perceptual_loss.lpips, "lpips.")
    tr.loss_huge_threshold = float("inf")
    return tr


@pytest.mark.parametrize("stage", [3, 1])
def test_graph_replay_equals_eager(stage):
    x = seeded_input("image", (2, 3, 64, 64)).to(dev())
    noise = {"y": seeded_input("noise.y", (2, 320, 4, 4), 0.5).to(dev()), "z": seeded_input("noise.z", (2, 192, 1, 1), 0.5).to(dev())}
    logs = {}
    params = {}
    for mode in (False, True):
        tr = _trainer(stage, mode)
        out = []
        for it in range(1, 6):
            data = {"real_images": x, "noise": noise}
            if stage == 3:
                data.update(rate_ind=1, beta=2.56 + 0.01 * it)  # beta changes every step: must flow through device buffers
            out.append(tr.optimize_parameters(it, data))
        if mode:
            assert len(tr.graphs) == (4 if stage == 3 else 2), "segments were not captured"  # g, dfb, u, d
        logs[mode] = out
        params[mode] = {k: p.detach().clone() for k, p in tr.comp_model.named_parameters()}
        if stage == 3:
            params[mode].update({"D." + k: p.detach().clone() for k, p in tr.discriminator.named_parameters()})
        del tr
    for a, b in zip(logs[False], logs[True]):
        assert a is not None and b is not None
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], (k, a[k], b[k])
    for k in params[False]:
        assert torch.equal(params[False][k], params[True][k]), k


def test_skip_gate_inside_graph():
    tr = _trainer(3, True)
    tr.loss_huge_threshold = 10000.0  # seeded weights give a loss far above it -> every iteration must be skipped
    x = seeded_input("image", (2, 3, 64, 64)).to(dev())
    before = {k: p.detach().clone() for k, p in tr.comp_model.named_parameters()}
    for it in range(1, 5):
        assert tr.optimize_parameters(it, {"real_images": x, "rate_ind": 2, "beta": 1.0}) is None
    for k, p in tr.comp_model.named_parameters():
        assert torch.equal(before[k], p.detach()), k
    for k, p in tr.discriminator.named_parameters():
        assert torch.isfinite(p).all()
    tr.g_optimizer.host_step_counts()
    assert tr.g_optimizer.param_groups[0]["step"] == 0


def test_filter_caches_created_after_capture_follow_the_replayed_updates():
    """Persistent F(4x4) filter caches are valid by the version counters of their weight packs, and those counters used to advance only when
    Python ran PackTable.refill -- which a captured optimiser segment does not.  A cache created AFTER the capture (an eager evaluation pass at
    another image size) was filled once, stamped, and then trusted forever while the replays went on updating the packs on the device.  Now
    SegmentGraphs.run calls the refill's host-side bookkeeping after every replay (batched.on_replay / PackTable._replayed): the packs' versions
    advance, a cache the replayed rebuild launch did not cover falls behind and re-transforms, and it joins the device table for the next
    replay.  Checked against a forced re-transform, bit for bit."""
    from crdr_amd.hip import ops, packs
    ops.PREFER_WINOGRAD = 4
    try:
        tr = _trainer(1, True)
        x = seeded_input("image", (2, 3, 64, 64)).to(dev())
        xe = seeded_input("eval image", (1, 3, 128, 128)).to(dev())
        noise = {"y": seeded_input("noise.y", (2, 320, 4, 4), 0.5).to(dev()), "z": seeded_input("noise.z", (2, 192, 1, 1), 0.5).to(dev())}
        for it in range(1, 5):
            assert tr.optimize_parameters(it, {"real_images": x, "noise": noise}) is not None
        assert len(tr.graphs) == 2
        n0 = len(packs._filter_cache)
        assert n0 > 0, "the warm-up created no F(4x4) filter cache: the test would be vacuous"
        def evaluate():
            with torch.no_grad():
                return tr.comp_model.run_model(xe, is_train=False)["fake_images"].clone()
        out1 = evaluate()
        assert len(packs._filter_cache) > n0, "the evaluation shapes created no new cache"
        st0 = dict(packs.FILTER_STATS)
        for it in range(5, 8):   # replays only: the packs change on the device
            assert tr.optimize_parameters(it, {"real_images": x, "noise": noise}) is not None
        out2 = evaluate()
        packs.drop_filter_caches()    # every cache dropped: the next pass transforms from the current packs
        out3 = evaluate()
        assert not torch.equal(out1, out2), "three optimiser steps must have moved the reconstruction"
        assert torch.equal(out2, out3), "an evaluation pass after graph replays ran on filters transformed from OLD weights"
        assert packs.FILTER_STATS["batched"] > st0["batched"] or packs.FILTER_STATS["filled"] > st0["filled"]
    finally:
        ops.PREFER_WINOGRAD = False
        packs.drop_filter_caches()


def test_eager_pass_after_capture_never_rewrites_the_replayed_colsum_table():
    """The column-sum job table of a captured chain backward is frozen (hip/batched.py): the captured conv launches write their partial rows
    to the addresses it held at capture time.  An eager pass of the same site with the same content leaves it alone and the next replay gives
    the same gradients bit for bit; an eager pass whose jobs differ -- one bias gradient lives at another address -- raises instead of
    changing what the graph computes."""
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    from crdr_amd.models.layer.elic_layers import ResidualBottleneckBlocks
    from crdr_amd.trainer.graphs import SegmentGraphs
    d = dev()
    torch.manual_seed(0)
    net = ResidualBottleneckBlocks(64, 32, num_blocks=2).to(d)
    params = list(net.parameters())
    for p in params:
        p.grad = torch.zeros_like(p)
    x = seeded_input("chain input", (2, 64, 16, 16)).to(d).contiguous(memory_format=torch.channels_last)
    q, site = ops.colsum_queue(d), net._chain(False).site
    defer = ops.DeferredWgrad(d, arena_bytes=64 << 20)   # (a queue of this test's own: its captured tables die with it)
    prev, ops.WGRAD_DEFER = ops.WGRAD_DEFER, defer

    def step():
        for p in params:
            p.grad.zero_()
        net(x).square().sum().backward()
        ops.flush_wgrads("frozen colsum table")

    def grads():
        torch.cuda.synchronize()
        return [p.grad.clone() for p in params]
    sg = SegmentGraphs(True)
    try:
        with sg.step_scope():
            step()
            step()
            g_eager = grads()
            assert all(float(g.abs().max()) > 0 for g in g_eager)
            sg.run("chain backward", step)
            g_graph = grads()
            for a, b in zip(g_eager, g_graph):
                assert torch.equal(a, b)
            twin = q.tables.tables[(site, True)]
            assert twin.replayed and not q.tables.tables[(site, False)].replayed
            held = [t.clone() for t in (twin.items, twin.prefix, twin.meta)]
            step()   # eager, same shapes: same jobs at the same addresses
            sg.run("chain backward", step)
            assert all(torch.equal(a, b) for a, b in zip(held, (twin.items, twin.prefix, twin.meta)))
            for a, b in zip(g_graph, grads()):
                assert torch.equal(a, b)
            bias = net.block0.conv[0].bias
            keep, bias.grad = bias.grad, torch.zeros_like(bias)   # its column sum now goes to another address
            try:
                with pytest.raises(L.CrdrHipError, match="re-capture the graphs"):
                    step()
            finally:
                q.drop()
                defer.drop()
                bias.grad = keep
            sg.run("chain backward", step)
            assert all(torch.equal(a, b) for a, b in zip(held, (twin.items, twin.prefix, twin.meta)))
            for a, b in zip(g_graph, grads()):
                assert torch.equal(a, b)
    finally:
        ops.WGRAD_DEFER = prev
