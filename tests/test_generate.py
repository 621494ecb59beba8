"""KV-cache generation on the CPU reference path: incremental decoding equals the full forward,
ragged prompts, the decode-attention and rope-append references, sampling, host-side validation,
checkpoint loading and the generate workload."""
import functools
import json

import pytest
import torch

from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig
from tensorhive_fixed_amd.ops.decode_attention import KVCache, decode_attention, rope_append
from tensorhive_fixed_amd.ops.rope import rope_reference_
from tests import decode_oracles as do

ULP = 2.0 ** -8  # bf16 spacing relative to the magnitude


@functools.lru_cache(maxsize=None)
def _tiny():
    cfg = LlamaConfig.tiny()
    model = Llama(cfg, device="cpu", seed=3)
    tokens = torch.randint(0, cfg.vocab_size, (2, 48), generator=torch.Generator().manual_seed(11))
    return cfg, model, tokens, model.logits(tokens).float()


def _incremental(model, tokens, lens, steps, max_len=64):
    """Teacher-forced logits [B, 1 + steps, vocab]: prefill at ``lens``, then one token at a time."""
    B = tokens.shape[0]
    cache = KVCache(model.cfg, B, max_len, tokens.device)
    prompt = torch.zeros((B, max(lens)), dtype=tokens.dtype, device=tokens.device)
    for b, n in enumerate(lens):
        prompt[b, :n] = tokens[b, :n]
    h = model.prefill(prompt, lens, cache)
    out = [torch.mm(h, model.lm_head.t()).float()]
    for i in range(steps):
        nxt = torch.stack([tokens[b, n + i] for b, n in enumerate(lens)])
        out.append(model.decode_step(nxt, cache))
    assert cache.lens == [n + steps for n in lens]
    assert cache.lens_dev.tolist() == cache.lens
    return torch.stack(out, dim=1)


def test_incremental_equals_full():
    _, model, tokens, full = _tiny()
    inc = _incremental(model, tokens, [17, 17], 31)
    ref = full[:, 16:48]
    err = (inc - ref).abs().max().item()
    bound = 4 * ULP * ref.abs().max().item()
    print(f"max |delta| {err:.4g}  bound {bound:.4g}")
    assert err <= bound


def test_ragged_prompts_equal_each_sequence_alone():
    _, model, tokens, _ = _tiny()
    lens, steps = [5, 17], 6
    both = _incremental(model, tokens, lens, steps)
    for b, n in enumerate(lens):
        alone = _incremental(model, tokens[b: b + 1], [n], steps)
        err = (both[b] - alone[0]).abs().max().item()
        assert err <= 4 * ULP * alone.abs().max().item(), (b, err)


@pytest.mark.parametrize("lens", do.KV_LENS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_decode_attention_reference_against_fp64(Hq, Hkv, lens):
    cache, q = do.nan_dead_cache(Hq, Hkv, lens, "cpu")
    do.assert_attention_close(decode_attention(q, cache, 0), do.attention_fp64(q, cache))


def test_rope_append_matches_rope_reference():
    Hq, Hkv, smax = 8, 2, 128
    cfg = do.attn_cfg(Hq, Hkv, n_layers=2, max_seq_len=smax)
    pos = [0, 77, smax - 1]
    cache = KVCache(cfg, 3, smax, "cpu")
    g = torch.Generator().manual_seed(5)
    cache.kv.copy_(torch.randn(cache.kv.shape, generator=g))
    cache.set_lens(pos)
    before = cache.kv.clone()
    qkv = torch.randn(3, (Hq + 2 * Hkv) * 128, generator=g).to(torch.bfloat16)
    q = rope_append(qkv, cache, 1)
    assert cache.lens == pos  # the model advances the lengths once all layers have appended
    for b, p in enumerate(pos):
        # rope_reference_ rotates row t at position t % S: put the row at t = p
        rows = torch.zeros(smax, qkv.shape[1], dtype=torch.bfloat16)
        rows[p] = qkv[b]
        ref = rope_reference_(rows, smax, Hq + Hkv, 128, cfg.rope_theta)[p]
        assert torch.equal(q[b], ref[: Hq * 128])
        assert torch.equal(cache.k(1)[b, :, p].reshape(-1), ref[Hq * 128: (Hq + Hkv) * 128])
        assert torch.equal(cache.v(1)[b, :, p].reshape(-1), qkv[b, (Hq + Hkv) * 128:])  # v bit-exact
    touched = torch.zeros(cache.kv.shape, dtype=torch.bool)
    for b, p in enumerate(pos):
        touched[1, :, b, :, p] = True
    assert torch.equal(cache.kv[~touched], before[~touched])


def _margin_logits():
    z = torch.randn(4, 50, generator=torch.Generator().manual_seed(2))
    z[torch.arange(4), torch.tensor([7, 0, 49, 21])] += 10.0
    return z


def test_sampling():
    z = _margin_logits()
    greedy = Llama.sample(z)
    assert greedy.tolist() == [7, 0, 49, 21]
    assert torch.equal(Llama.sample(z, temperature=0.0), greedy)
    assert torch.equal(Llama.sample(z, temperature=1.3, top_k=1), greedy)
    draws = [Llama.sample(z, temperature=5.0, top_k=20, generator=torch.Generator().manual_seed(9))
             for _ in range(2)]
    assert torch.equal(draws[0], draws[1])
    kept = z.topk(20, dim=-1).indices
    assert all(int(t) in kept[b].tolist() for b, t in enumerate(draws[0]))


def test_generate_is_deterministic_and_reproducible():
    cfg, model, tokens, _ = _tiny()
    a, la = model.generate(tokens[:, :17], max_new_tokens=4, return_logits=True)
    b = model.generate(tokens[:, :17], max_new_tokens=4)
    assert a.shape == (2, 4) and la.shape == (2, 4, cfg.vocab_size) and la.dtype == torch.float32
    assert torch.equal(a, b) and int(a.min()) >= 0 and int(a.max()) < cfg.vocab_size
    assert torch.equal(a, la.argmax(-1))
    s1 = model.generate(tokens[:, :17], [5, 17], max_new_tokens=4, temperature=1.0, top_k=8,
                        generator=torch.Generator().manual_seed(4))
    s2 = model.generate(tokens[:, :17], [5, 17], max_new_tokens=4, temperature=1.0, top_k=8,
                        generator=torch.Generator().manual_seed(4))
    assert torch.equal(s1, s2)


def test_add_norm_flow_is_required(monkeypatch):
    from tensorhive_fixed_amd.models import llama3

    _, model, tokens, _ = _tiny()
    monkeypatch.setattr(llama3, "ADD_NORM", False)
    with pytest.raises(RuntimeError, match="TH_ADD_NORM"):
        model.decode_step(tokens[:, 0], KVCache(model.cfg, 2, 8, "cpu"))


def test_validation_raises_before_any_launch():
    cfg = do.attn_cfg(4, 2, max_seq_len=32)
    with pytest.raises(ValueError):
        KVCache(cfg, 2, 33, "cpu")  # max_len > cfg.max_seq_len
    with pytest.raises(ValueError):
        KVCache(LlamaConfig(dim=256, n_heads=4, n_kv_heads=2, max_seq_len=32, n_layers=1), 2, 16, "cpu")  # Dh 64
    with pytest.raises(ValueError):
        KVCache(LlamaConfig(dim=384, n_heads=3, n_kv_heads=2, max_seq_len=32, n_layers=1), 2, 16, "cpu")  # Hq % Hkv
    cache = KVCache(cfg, 2, 16, "cpu")
    q = torch.zeros(2, 4 * 128, dtype=torch.bfloat16)
    qkv = torch.zeros(2, 8 * 128, dtype=torch.bfloat16)
    cache.set_lens([3, 16])
    with pytest.raises(ValueError):
        rope_append(qkv, cache, 0)  # 16 + 1 > max_len
    with pytest.raises(ValueError):
        decode_attention(q, cache, 0, new=1)
    decode_attention(q, cache, 0)  # 16 rows fit
    with pytest.raises(ValueError):
        cache.advance(1)
    with pytest.raises(ValueError):
        cache.set_lens([3, 17])
    cache.set_lens([3, 4])
    for bad in (q.float(), torch.zeros(2, 8 * 128, dtype=torch.bfloat16)[:, : 4 * 128], q[:1],
                torch.zeros(2, 3 * 128, dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            decode_attention(bad, cache, 0)
    for bad in (qkv.float(), torch.zeros(2, 9 * 128, dtype=torch.bfloat16)[:, : 8 * 128], q):
        with pytest.raises(ValueError):
            rope_append(bad, cache, 0)
    with pytest.raises(ValueError):
        decode_attention(q, cache, 1)  # no such layer
    with pytest.raises(ValueError):
        decode_attention(q, cache, 0, nsplit=0)


def _tiny_checkpoint(tmp_path):
    from tensorhive_fixed_amd.workloads import llama3_ddp

    assert llama3_ddp.main(["--model", "tiny", "--seq-len", "16", "--micro-batch", "1", "--steps", "1",
                            "--warmup", "0", "--log-every", "100", "--ckpt-dir", str(tmp_path),
                            "--ckpt-every", "1"]) == 0
    return str(tmp_path / "ckpt.pt")


def test_load_checkpoint_params_round_trip(tmp_path, monkeypatch):
    from tensorhive_fixed_amd.parallel.flat import FlatParamStore
    from tensorhive_fixed_amd.workloads.llama3_generate import load_checkpoint_params

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    path = _tiny_checkpoint(tmp_path)
    st = torch.load(path, weights_only=True)
    model = Llama(LlamaConfig.tiny(), device="cpu", seed=99)
    load_checkpoint_params(model, path)
    assert not hasattr(model.tok_emb, "main_grad")  # no gradient / optimizer buffers came with it
    # the trained parameters, as a store of the same model lays them out
    other = Llama(LlamaConfig.tiny(), device="cpu", seed=1)
    store = FlatParamStore(other.params_in_backward_order(), torch.device("cpu"))
    store.param_buf.copy_(st["param_buf"])
    for (name, p, _), (_, ref, _) in zip(model.params_in_backward_order(), other.params_in_backward_order()):
        assert torch.equal(p, ref), name
    st["names"] = "something.else"
    torch.save(st, path)
    with pytest.raises(ValueError):
        load_checkpoint_params(model, path)


def test_generate_workload_emits_done(tmp_path, capsys):
    from tensorhive_fixed_amd.workloads import llama3_generate

    prompts = tmp_path / "prompts.json"
    prompts.write_text(json.dumps([[1, 2, 3, 4, 5], [7] * 17]))
    assert llama3_generate.main(["--model", "tiny", "--device", "cpu", "--prompt-ids", str(prompts),
                                 "--max-new-tokens", "5", "--log-every", "2", "--temperature", "0.8",
                                 "--top-k", "4", "--seed", "3"]) == 0
    out = capsys.readouterr().out.splitlines()
    done = json.loads(out[-1])
    assert done["event"] == "done" and done["new_tokens"] == 10
    assert done["prefill_ms"] > 0 and done["decode_ms_per_token"] > 0
    assert any(line.startswith("[th-gen] step=") and "tokens/s=" in line and "batch=2" in line for line in out)
    assert llama3_generate.main(["--model", "tiny", "--device", "cpu", "--batch", "2", "--prompt-len", "9",
                                 "--max-new-tokens", "2"]) == 0
    assert json.loads(capsys.readouterr().out.splitlines()[-1])["new_tokens"] == 4
