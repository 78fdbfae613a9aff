"""The launch sequence of one training step, pinned: the entry points of the kernel library that one clm_loss forward
plus backward calls, in order, for every way a transformer block's two halves are built today -- the plain pre-norm
block (ModelForCausalLM, key-padding mask), Qwen3Model with and without qk_norm, LoRA adapters on some or all
projections over a frozen embedding (layer 0 skips its input gradient), and the post-LN decoder layer (SelfAttentionFn).
The pre-norm models run under plain autograd (gradients returned) and under FlatTrainer (gradients accumulated into the
arena; at these row counts every weight gradient is its own launch -- the grouped route is pinned by the
grouped-versus-ungrouped tests).

Every ops wrapper launches through _lib.call, which ops binds by from-import: both names are wrapped, and only the
names of host-side calls are counted.  vy_workspace_set is left out: a stream's scratch is registered once per process,
so whether a test sees it depends on the tests before it.  The expected lists were recorded before the block functions
were gathered into one core and must not change with it: same kernels, same order."""
import pytest
import torch

from tests.golden import cases
from tests.golden import cases_causal_lm as C
from tests.golden import cases_lora as L
from tests.golden import cases_qwen3_train as Q
from vyomai_amd import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(a):
    return torch.from_numpy(a).to(DEV)


@pytest.fixture
def trace(monkeypatch):
    from vyomai_amd import _lib, ops
    names = []
    real = _lib.call

    def spy(name, *args):
        if name != "vy_workspace_set":
            names.append(name[3:])
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    monkeypatch.setattr(ops, "call", spy)
    return names


def step(trace, key, model, loss_fn, mode):
    """One forward + backward of a fresh model -> checked against EXPECT[key]."""
    if mode == "trainer":
        from vyomai_amd.training import FlatTrainer
        tr = FlatTrainer(model, lr=C.LR, weight_decay=C.WEIGHT_DECAY, overlap_optimizer=False)
        tr.zero_grad()
        del trace[:]
        tr.backward(loss_fn())
    else:
        del trace[:]
        loss_fn().backward()
    torch.cuda.synchronize()
    got = list(trace)
    print(f"{key}: {' '.join(got)}")
    assert got == EXPECT[key], key


MODES = ("autograd", "trainer")


@pytest.mark.parametrize("mode", MODES)
def test_causal_lm_with_key_padding(trace, mode):
    from tests.test_causal_lm_gpu import build
    m = build(C.CASES["a"]).train()
    ids, mask, labels = (T(a) for a in C.padded_batch("a"))
    step(trace, f"clm.{mode}", m, lambda: m.clm_loss(ids, labels, mask), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["q", "n"])       # with qk_norm, without
def test_qwen3(trace, case, mode):
    import vyomai_amd as V
    assert Q.CASES["q"]["qk_norm"] and not Q.CASES["n"]["qk_norm"]
    m = Q.build(V.Qwen3Model, case, torch.float32).to(DEV).train()
    ids, mask, labels = (T(a) for a in Q.train_batch(case))
    step(trace, f"qwen3.{case}.{mode}", m, lambda: m.clm_loss(ids, labels), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("who", tuple(L.ADAPTERS))
def test_lora(trace, who, mode):
    from tests.test_lora_train_gpu import wrapped
    m = wrapped(who).train()
    ids, mask, labels = (T(a) for a in C.padded_batch(L.CASE))
    step(trace, f"lora.{who}.{mode}", m, lambda: m.clm_loss(ids, labels, mask), mode)


def test_post_ln_decoder(trace):
    """The 2-layer post-LN decoder of test_training_gpu.py's trainer test."""
    import vyomai_amd as V
    cfg = cases.test_cfg()
    cfg.num_hidden_layers, cfg.vocab_size, cfg.hidden_dropout_prob = 2, 1031, 0.0
    m = V.DecoderModel(cfg, "rope", None)
    recipe.load_recipe_(m)
    m = m.to(DEV).train()
    ids = torch.from_numpy(recipe.token_ids("train.ids", (4, 48), 3, cfg.vocab_size)).to(DEV)
    labels = ids.clone()
    labels[0, 40:] = -100
    step(trace, "post_ln", m, lambda: m.clm_loss(ids, labels), "autograd")


EXPECT = {
    "clm.autograd": """
        embedding_fwd rmsnorm_fwd qkv_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd gated_act_fwd linear_fwd
        rmsnorm_fwd qkv_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd gated_act_fwd linear_fwd rmsnorm_fwd
        linear_fwd xent_fwd xent_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad
        gated_act_fwd linear_wgrad gated_act_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose
        linear_dgrad linear_wgrad attn_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad
        gated_act_fwd linear_wgrad gated_act_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose
        linear_dgrad linear_wgrad attn_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd embedding_bwd
    """.split(),
    "clm.trainer": """
        embedding_fwd rmsnorm_fwd qkv_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd gated_act_fwd linear_fwd
        rmsnorm_fwd qkv_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd gated_act_fwd linear_fwd rmsnorm_fwd
        linear_fwd xent_fused transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad gated_act_fwd
        linear_wgrad gated_act_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad
        linear_wgrad attn_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad gated_act_fwd
        linear_wgrad gated_act_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad
        linear_wgrad attn_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd embedding_bwd
    """.split(),
    "qwen3.q.autograd": """
        embedding_fwd rmsnorm_fwd linear_fwd qknorm_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd
        gated_act_fwd linear_fwd rmsnorm_fwd linear_fwd qknorm_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd
        gated_act_fwd linear_fwd rmsnorm_fwd linear_fwd xent_fwd xent_bwd transpose linear_dgrad linear_wgrad
        rmsnorm_bwd transpose linear_dgrad gated_act_fwd linear_wgrad gated_act_bwd transpose linear_dgrad
        linear_wgrad rmsnorm_bwd transpose linear_dgrad linear_wgrad attn_bwd qknorm_bwd transpose linear_dgrad
        linear_wgrad rmsnorm_bwd transpose linear_dgrad gated_act_fwd linear_wgrad gated_act_bwd transpose
        linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad linear_wgrad attn_bwd qknorm_bwd transpose
        linear_dgrad linear_wgrad rmsnorm_bwd embedding_bwd
    """.split(),
    "qwen3.q.trainer": """
        embedding_fwd rmsnorm_fwd linear_fwd qknorm_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd
        gated_act_fwd linear_fwd rmsnorm_fwd linear_fwd qknorm_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd
        gated_act_fwd linear_fwd rmsnorm_fwd linear_fwd xent_fused transpose linear_dgrad linear_wgrad rmsnorm_bwd
        transpose linear_dgrad gated_act_fwd linear_wgrad gated_act_bwd transpose linear_dgrad linear_wgrad
        rmsnorm_bwd transpose linear_dgrad linear_wgrad attn_bwd qknorm_bwd transpose linear_dgrad linear_wgrad
        rmsnorm_bwd transpose linear_dgrad gated_act_fwd linear_wgrad gated_act_bwd transpose linear_dgrad
        linear_wgrad rmsnorm_bwd transpose linear_dgrad linear_wgrad attn_bwd qknorm_bwd transpose linear_dgrad
        linear_wgrad rmsnorm_bwd embedding_bwd
    """.split(),
    "qwen3.n.autograd": """
        embedding_fwd rmsnorm_fwd qkv_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd gated_act_fwd linear_fwd
        rmsnorm_fwd qkv_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd gated_act_fwd linear_fwd rmsnorm_fwd
        linear_fwd xent_fwd xent_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad
        gated_act_fwd linear_wgrad gated_act_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose
        linear_dgrad linear_wgrad attn_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad
        gated_act_fwd linear_wgrad gated_act_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose
        linear_dgrad linear_wgrad attn_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd embedding_bwd
    """.split(),
    "qwen3.n.trainer": """
        embedding_fwd rmsnorm_fwd qkv_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd gated_act_fwd linear_fwd
        rmsnorm_fwd qkv_rope_fwd attn_fwd linear_fwd rmsnorm_fwd linear_fwd gated_act_fwd linear_fwd rmsnorm_fwd
        linear_fwd xent_fused transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad gated_act_fwd
        linear_wgrad gated_act_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad
        linear_wgrad attn_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad gated_act_fwd
        linear_wgrad gated_act_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd transpose linear_dgrad
        linear_wgrad attn_bwd transpose linear_dgrad linear_wgrad rmsnorm_bwd embedding_bwd
    """.split(),
    "lora.n1.autograd": """
        embedding_fwd rmsnorm_fwd linear_fwd lora_shrink lora_expand rope_fwd rope_fwd attn_fwd linear_fwd
        lora_shrink lora_expand rmsnorm_fwd linear_fwd lora_shrink lora_expand gated_act_fwd linear_fwd lora_shrink
        lora_expand rmsnorm_fwd linear_fwd lora_shrink lora_expand rope_fwd rope_fwd attn_fwd linear_fwd lora_shrink
        lora_expand rmsnorm_fwd linear_fwd lora_shrink lora_expand gated_act_fwd linear_fwd lora_shrink lora_expand
        rmsnorm_fwd linear_fwd xent_fwd xent_bwd transpose linear_dgrad rmsnorm_bwd transpose linear_dgrad
        gated_act_fwd lora_shrink lora_expand lora_wgrad gated_act_bwd transpose linear_dgrad lora_shrink
        lora_expand lora_wgrad rmsnorm_bwd transpose linear_dgrad lora_shrink lora_expand lora_wgrad attn_bwd
        transpose linear_dgrad lora_shrink lora_expand lora_wgrad rmsnorm_bwd transpose linear_dgrad gated_act_fwd
        lora_shrink lora_expand lora_wgrad gated_act_bwd transpose linear_dgrad lora_shrink lora_expand lora_wgrad
        rmsnorm_bwd transpose linear_dgrad lora_shrink lora_expand lora_wgrad attn_bwd lora_shrink lora_wgrad
    """.split(),
    "lora.n1.trainer": """
        embedding_fwd rmsnorm_fwd linear_fwd lora_shrink lora_expand rope_fwd rope_fwd attn_fwd linear_fwd
        lora_shrink lora_expand rmsnorm_fwd linear_fwd lora_shrink lora_expand gated_act_fwd linear_fwd lora_shrink
        lora_expand rmsnorm_fwd linear_fwd lora_shrink lora_expand rope_fwd rope_fwd attn_fwd linear_fwd lora_shrink
        lora_expand rmsnorm_fwd linear_fwd lora_shrink lora_expand gated_act_fwd linear_fwd lora_shrink lora_expand
        rmsnorm_fwd linear_fwd xent_fused transpose linear_dgrad rmsnorm_bwd transpose linear_dgrad gated_act_fwd
        lora_shrink lora_expand lora_wgrad gated_act_bwd transpose linear_dgrad lora_shrink lora_expand lora_wgrad
        rmsnorm_bwd transpose linear_dgrad lora_shrink lora_expand lora_wgrad attn_bwd transpose linear_dgrad
        lora_shrink lora_expand lora_wgrad rmsnorm_bwd transpose linear_dgrad gated_act_fwd lora_shrink lora_expand
        lora_wgrad gated_act_bwd transpose linear_dgrad lora_shrink lora_expand lora_wgrad rmsnorm_bwd transpose
        linear_dgrad lora_shrink lora_expand lora_wgrad attn_bwd lora_shrink lora_wgrad
    """.split(),
    "post_ln": """
        embedding_fwd qkv_rope_fwd attn_fwd linear_fwd layernorm_fwd linear_fwd linear_fwd layernorm_fwd
        qkv_rope_fwd attn_fwd linear_fwd layernorm_fwd linear_fwd linear_fwd layernorm_fwd linear_fwd layernorm_fwd
        linear_fwd xent_fwd xent_bwd transpose linear_dgrad linear_wgrad layernorm_bwd act_bwd transpose
        linear_dgrad linear_wgrad layernorm_bwd transpose linear_dgrad linear_wgrad transpose linear_dgrad
        linear_wgrad layernorm_bwd transpose linear_dgrad linear_wgrad attn_bwd transpose linear_dgrad linear_wgrad
        layernorm_bwd transpose linear_dgrad linear_wgrad transpose linear_dgrad linear_wgrad layernorm_bwd
        transpose linear_dgrad linear_wgrad attn_bwd transpose linear_dgrad linear_wgrad embedding_bwd
    """.split(),
}
# the adapter n2 adds k_proj to n1's projections: a part of the packed qkv group, not one more launch
EXPECT["lora.n2.autograd"], EXPECT["lora.n2.trainer"] = EXPECT["lora.n1.autograd"], EXPECT["lora.n1.trainer"]
