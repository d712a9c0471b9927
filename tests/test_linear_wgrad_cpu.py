"""ops/linear.py without a GPU: the dw bound of linear_wgrad_refs.py can
fail (one-edge mutants fall outside it, the honest fp32 result inside), the
new path never engages on the CPU, so an engine step is bit-identical with
the switch on and off, and ZeRO-3 on two gloo ranks still trains with the
re-classed layers."""
import pytest
import torch
import torch.nn.functional as F

from edge_refs import assert_within
from linear_wgrad_refs import CASES, dw_reference, make_inputs
from tests.common import run_distributed


@pytest.mark.parametrize("T,K,N", CASES)
def test_bound_holds_for_an_fp32_sum(T, K, N):
    x, w, dy = make_inputs(T, K, N, "cpu")
    ref, tol = dw_reference(x, dy)
    dw = (dy.float().t() @ x.float()).to(torch.bfloat16)
    assert_within(dw, ref, tol, "fp32 dw")


def test_bound_rejects_one_edge_mutants():
    # x shifted by one row: every product pairs the wrong token
    x, w, dy = make_inputs(130, 72, 40, "cpu")
    ref, tol = dw_reference(x, dy)
    shifted = (dy.float().t() @ torch.roll(x.float(), 1, 0)).to(torch.bfloat16)
    with pytest.raises(AssertionError):
        assert_within(shifted, ref, tol, "dw from x shifted by a row")
    # square case: dw transposed has the right shape and the wrong layout
    x, w, dy = make_inputs(130, 72, 72, "cpu")
    ref, tol = dw_reference(x, dy)
    good = (dy.float().t() @ x.float()).to(torch.bfloat16)
    assert_within(good, ref, tol, "fp32 dw")
    with pytest.raises(AssertionError):
        assert_within(good.t().contiguous(), ref, tol, "dw transposed")


def test_cpu_never_takes_the_function(monkeypatch):
    from deepspeed_amd.ops import linear as L

    def boom(*a):
        raise AssertionError("the wgrad Function engaged on the CPU")

    monkeypatch.setattr(L._LinearWgradFn, "apply", staticmethod(boom))
    monkeypatch.setattr(L, "MIN_TOKENS", 1)
    monkeypatch.setattr(L, "WGRAD_ARRANGEMENT", {(40, 72): (True, True)})
    x, w, dy = make_inputs(130, 72, 40, "cpu")
    w.requires_grad_(True)
    y = L.linear(x, w)
    y.backward(dy)
    w0 = w.detach().clone().requires_grad_(True)
    F.linear(x, w0).backward(dy)
    assert torch.equal(w.grad, w0.grad)


def _tiny_step(switch):
    import os
    import torch.distributed as tdist
    import deepspeed_amd
    from deepspeed_amd.comm import groups
    from deepspeed_amd.models.llama import LLAMA_CONFIGS, LlamaForCausalLM
    from deepspeed_amd.ops.linear import WgradLinear
    assert not torch.cuda.is_available()
    os.environ["DSAMD_WGRAD_TN"] = switch
    groups.reset_groups()
    cfg = LLAMA_CONFIGS["llama-tiny"]
    torch.manual_seed(11)
    model = LlamaForCausalLM(cfg)
    names = list(model.state_dict())
    engine, _, _, _ = deepspeed_amd.initialize(model=model, config={
        "train_micro_batch_size_per_gpu": 2,
        "optimizer": {"type": "AdamW", "params": {"lr": 3e-4}},
        "zero_optimization": {"stage": 3},
        "bf16": {"enabled": True}})
    assert list(model.state_dict()) == names
    assert type(model.lm_head) is WgradLinear
    torch.manual_seed(5 + tdist.get_rank())
    data = torch.randint(0, cfg.vocab_size, (2, 32))
    losses = []
    for _ in range(3):
        loss = engine(data, labels=data)
        engine.backward(loss)
        engine.step()
        losses.append(loss.item())
    shard = next(iter(engine.module.parameters())).ds_tensor.detach() \
        .float().clone()
    engine.destroy()
    return losses, shard


@pytest.fixture
def cpu_children(monkeypatch):
    """These two tests are about the CPU: their spawned ranks see no GPU
    even on a machine that has one, so gloo only ever gets CPU tensors."""
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")


def test_engine_step_bit_identical_with_switch_on_and_off_world1(
        cpu_children):
    on = run_distributed(_tiny_step, world_size=1, backend="gloo",
                         args=("1",))[0]
    off = run_distributed(_tiny_step, world_size=1, backend="gloo",
                          args=("0",))[0]
    assert on[0] == off[0]
    assert torch.equal(on[1], off[1])


def test_zero3_two_gloo_ranks_still_train(cpu_children):
    for losses, _ in run_distributed(_tiny_step, world_size=2,
                                     backend="gloo", args=("1",)):
        assert losses[-1] < losses[0], losses
