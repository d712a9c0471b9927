"""ZeRO-3 store-first gradient accumulation: the first accumulate of a
parameter in a window overwrites its fp32 shard range instead of adding onto
a zero fill. The weights must be exactly those of fill-then-add, with a
parameter that never gets a gradient, one used twice in forward, and one
that gets gradients in the first window only (its range holds stale data in
the later windows and must read as zero)."""
import torch

import deepspeed_amd
from tests.common import run_distributed
from tests.simple_model import SimpleModel, make_batches

HIDDEN = 32
LR = 1e-2
WD = 0.5
STEPS = 3
GA = 2


class _Model(SimpleModel):
    def __init__(self):
        super().__init__(HIDDEN, nlayers=2)
        self.unused = torch.nn.Linear(HIDDEN, HIDDEN)       # never in forward
        self.sometimes = torch.nn.Linear(HIDDEN, HIDDEN)    # first window only
        self.use_sometimes = True

    def forward(self, x, y):
        h = x
        for l in (self.linears[0], self.linears[1], self.linears[0]):
            h = torch.nn.functional.gelu(l(h))              # [0] used twice
        if self.use_sometimes:
            h = h + self.sometimes(h)
        return self.loss_fn(self.norm(h), y)


def _train(store_first):
    import torch.distributed as dist
    from deepspeed_amd.utils import (safe_get_full_fp32_param,
                                     safe_get_full_grad)
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.manual_seed(11)
    model = _Model()
    config = {
        "train_micro_batch_size_per_gpu": 4,
        "gradient_accumulation_steps": GA,
        "optimizer": {"type": "AdamW",
                      "params": {"lr": LR, "weight_decay": WD}},
        "zero_optimization": {"stage": 3, "reduce_bucket_size": 2000,
                              "stage3_param_persistence_threshold": 10,
                              "sub_group_size": 1500},
        "bf16": {"enabled": True},
    }
    engine, _, _, _ = deepspeed_amd.initialize(model=model, config=config)
    opt = engine.optimizer
    opt._set_store_first(store_first)
    assert all(sg.store_first == store_first for sg in opt.sub_groups)
    params = dict(model.named_parameters())

    def masters():
        return {n: safe_get_full_fp32_param(p, opt).detach().cpu().clone()
                for n, p in params.items()}

    batches = make_batches(STEPS * GA * world, 4, HIDDEN,
                           dtype=torch.bfloat16)
    snaps = [masters()]
    grads = []
    i = 0
    for s in range(STEPS):
        model.use_sometimes = s == 0
        for g in range(GA):
            x, y = batches[i * world + rank]
            engine.backward(engine(x, y))
            if g == GA - 1:
                # a reader between backward and step sees finished grads
                grads.append({n: safe_get_full_grad(p, opt).detach().cpu()
                              .clone() for n, p in params.items()})
            engine.step()
            i += 1
        snaps.append(masters())
    return snaps, grads


def _both():
    return _train(True), _train(False)


def test_store_first_equals_fill_then_add():
    world = 2
    for (new, gnew), (old, gold) in run_distributed(_both, world_size=world):
        assert len(new) == STEPS + 1
        for s in range(STEPS + 1):
            for n in new[s]:
                assert torch.equal(new[s][n], old[s][n]), (s, n)
        for s in range(STEPS):
            for n in gnew[s]:
                assert torch.equal(gnew[s][n], gold[s][n]), (s, n)
        # parameters that got no gradient in a window read as exactly zero
        for s in range(STEPS):
            assert not gnew[s]["unused.weight"].any()
            if s > 0:
                assert not gnew[s]["sometimes.weight"].any()
        assert gnew[0]["sometimes.weight"].any()
        assert gnew[0]["linears.0.weight"].any()
        # the never-used parameter moves by weight decay only
        for n in ("unused.weight", "unused.bias"):
            want = new[0][n].clone()
            for s in range(STEPS):
                want = want * (1.0 - LR * WD)
                assert torch.allclose(new[s + 1][n], want, rtol=1e-6,
                                      atol=0.0), (s, n)
            assert not torch.equal(new[STEPS][n], new[0][n])
