"""Generate tests/golden/lora.npz by running the REAL reference: its ModelForCausalLM (VyomAI/models/custom_transformer.py;
needs `transformers`), case "a" filled by cases_causal_lm.load_weights_, with its linears wrapped by the reference's
LoraLinear (VyomAI/layers/adapters.py) as Examples/adapters.ipynb wraps them, on the CPU in fp32.  The reference is
imported at run time only; only inputs and outputs are stored.  This repository goes BEFORE the reference on the path
(the reference has a `tests` package of its own):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<this repository>:<reference checkout> python tests/golden/make_golden_lora.py

Keys (who = base | n1 | n2, see cases_lora.py):
  <adapter>.keys, <adapter>.w.<key>     the adapter's tensors under the reference's state_dict key names (fp16: exact)
  <who>.steps                           logits of prefill(8) + 8 single-token steps through DynamicCache, (B, 9, V)
  prompt, prompt.seed                   (B, 8) prompts, shared by base and both adapters
  <who>.greedy, <who>.greedy.logits     8 greedy ids per prompt and the logits rows that decided them (B, 8, V)
  long, long.seed                       one 21-token prompt
  <who>.long.greedy, <who>.long.logits  its 8 greedy ids and their logits rows (8, V)
Asserted here (if one fails, change the adapter values, not the bar): every top-2 margin > 1e-3; each adapter's greedy
ids differ from the base's; the reference's own bf16 forward with n1 stays within rel_err 3e-2 of its fp32 one; the
reference's re-associated fp32 computation (W + alpha * lora_b @ lora_a merged into the weight) stays within rel_err
2e-5 of the wrapped one -- the fp32 bar of the engine test is attainable by the reference alone; the file < 1 MB.

Qwen3Model has no importable reference class, and no golden here: the engine test holds it against a merged-weight
copy of the model."""
import os
import sys

os.environ["MKL_CBWR"] = "COMPATIBLE"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from transformers.cache_utils import DynamicCache  # noqa: E402
from VyomAI.layers.adapters import LoraLinear  # noqa: E402  (the reference)
from VyomAI.models import custom_transformer as ref  # noqa: E402  (the reference)
from tests.golden import cases_causal_lm as C  # noqa: E402
from tests.golden import cases_lora as L  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(got, want):
    got, want = got.detach().float().numpy(), want.detach().float().numpy()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def base():
    m = ref.ModelForCausalLM(ref.Config(**L.KW)).eval()
    C.load_weights_(m)
    return m


def spot(m, key):
    """-> (the module that owns the linear `key` names, its attribute name)."""
    parts = key.split(".")
    owner = m
    for p in parts[:-1]:
        owner = getattr(owner, p)
    return owner, parts[-1]


def wrapped(who):
    """The base model with the adapter's linears replaced by the reference's LoraLinear."""
    m = base()
    if who == "base":
        return m
    spec, state = L.ADAPTERS[who], L.adapter_state(who)
    for key in sorted({k.rsplit(".", 1)[0] for k in state}):
        owner, attr = spot(m, key)
        lora = LoraLinear(getattr(owner, attr), rank=spec["rank"], alpha=spec["alpha"])
        with torch.no_grad():
            lora.lora_a.copy_(T(state[key + ".lora_a"]))
            lora.lora_b.copy_(T(state[key + ".lora_b"]))
        setattr(owner, attr, lora)
    assert set(state) <= set(m.state_dict()), "the stored keys are the wrapped model's own state_dict keys"
    return m.eval()


def merged(who):
    """The re-associated computation: W + alpha * lora_b @ lora_a in the base model's own linears."""
    m = base()
    spec, state = L.ADAPTERS[who], L.adapter_state(who)
    with torch.no_grad():
        for key in sorted({k.rsplit(".", 1)[0] for k in state}):
            owner, attr = spot(m, key)
            getattr(owner, attr).weight += spec["alpha"] * T(state[key + ".lora_b"]) @ T(state[key + ".lora_a"])
    return m


def steps(m, ids):
    with torch.no_grad():
        cache = DynamicCache()
        rows = [m(input_ids=ids[:, :L.PREFILL], past_key_values=cache, use_cache=True).logits[:, -1:]]
        for t in range(L.PREFILL, L.PREFILL + L.STEPS):
            rows.append(m(input_ids=ids[:, t:t + 1], past_key_values=cache, use_cache=True).logits)
    return torch.cat(rows, dim=1)


def greedy(m, prompt):
    """-> (ids (B, NEW), the logits rows that decided them (B, NEW, V), smallest top-2 margin)."""
    cache, cur, new, rows, margin = DynamicCache(), prompt, [], [], np.inf
    with torch.no_grad():
        for _ in range(L.NEW):
            lg = m(input_ids=cur, past_key_values=cache, use_cache=True).logits[:, -1]
            top = lg.topk(2, dim=-1).values
            margin = min(margin, float((top[:, 0] - top[:, 1]).min()))
            cur = lg.argmax(-1, keepdim=True)
            new.append(cur)
            rows.append(lg)
    return torch.cat(new, dim=1), torch.stack(rows, dim=1), margin


def pick(models, prompt_of, what):
    """The first seed whose prompt every model decides by more than 1e-3 at every step, and on which every adapter's
    ids differ from the base's."""
    for seed in range(64):
        prompt = T(prompt_of(seed))
        prompt = prompt[None] if prompt.dim() == 1 else prompt
        runs = {who: greedy(m, prompt) for who, m in models.items()}
        margin = min(r[2] for r in runs.values())
        moved = all(bool((runs[who][0] != runs["base"][0]).any()) for who in L.ADAPTERS)
        if margin > 1e-3 and moved:
            print(f"{what}: seed {seed}, smallest top-2 margin {margin:.3e}")
            return seed, prompt, runs
    raise AssertionError(f"{what}: no seed with every margin > 1e-3 and moved ids")


def main():
    out = {}
    models = {who: wrapped(who) for who in L.WHO}
    ids = T(L.ids())
    for who in L.ADAPTERS:
        state = L.adapter_state(who)
        out[f"{who}.keys"] = np.array(sorted(state))
        for k, v in state.items():
            assert np.array_equal(v.astype(np.float16).astype(np.float32), v), k
            assert np.abs(v).max() > 0, k
            out[f"{who}.w.{k}"] = v.astype(np.float16)
    for who, m in models.items():
        out[f"{who}.steps"] = steps(m, ids).numpy()
    for who in L.ADAPTERS:
        moved = rel_err(T(out[f"{who}.steps"]), T(out["base.steps"]))
        # the re-associated fp32 computation: the fp32 bar of the engine test is attainable by the reference alone
        gap = rel_err(steps(merged(who), ids), T(out[f"{who}.steps"]))
        print(f"{who}: logits moved by rel_err {moved:.3f} against the base; merged-weight fp32 gap {gap:.2e}")
        assert moved > 0.1 and gap < 2e-5, (moved, gap)
    with torch.no_grad():
        full = models["n1"](input_ids=ids, use_cache=False).logits
        half = wrapped("n1").to(torch.bfloat16)(input_ids=ids, use_cache=False).logits
    gap = rel_err(half, full)
    print(f"n1: reference bf16 vs fp32 logits {gap:.2e}")
    assert gap < 3e-2, gap
    seed, prompt, runs = pick(models, L.prompts, "prompts")
    out["prompt"], out["prompt.seed"] = prompt.numpy(), np.array([seed], dtype=np.int64)
    for who, (new, rows, _) in runs.items():
        out[f"{who}.greedy"], out[f"{who}.greedy.logits"] = new.numpy(), rows.numpy()
    seed, prompt, runs = pick(models, L.long_prompt, "long prompt")
    out["long"], out["long.seed"] = prompt[0].numpy(), np.array([seed], dtype=np.int64)
    for who, (new, rows, _) in runs.items():
        out[f"{who}.long.greedy"], out[f"{who}.long.logits"] = new[0].numpy(), rows[0].numpy()
    path = os.path.join(HERE, "lora.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
