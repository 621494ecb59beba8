"""Llama-3 bf16 generation payload: load a training checkpoint (or random-init weights) and produce
tokens with the KV cache and the split-KV decode attention kernel (``ops/decode_attention.py``).

Launched like the training payload, one process on one GPU (``python -m
tensorhive_fixed_amd.workloads.llama3_generate``), typically as a task of the tensorhive job queue.
It prints ``[th-gen] step=N tokens/s=X batch=B`` lines and ends with one JSON line
``{"event": "done", "new_tokens": ..., "prefill_ms": ..., "decode_ms_per_token": ..., "stream_gemm": ...,
"graph": ..., "fp8_weights": ..., "quantize_ms": ..., "kv_dtype": ..., "kv_cache_mb": ...}``.
``--stream-gemm`` runs the decode steps' GEMMs on the weight-streaming kernel of ``ops/decode_linear.py``;
``--graph`` captures the decode step once and replays it for every token (``models/decode_graph.py``;
the capture happens right after the prefill and is counted in ``prefill_ms``).  The two compose.
``--fp8-weights`` quantizes the decode-step weights to FP8 after the checkpoint load (``quantize_ms``, not
counted in ``prefill_ms``) and runs every decode-step GEMM on them (``ops/decode_linear_fp8.py``, batch <= 16);
it composes with ``--graph`` and takes precedence over ``--stream-gemm``.
``--fp8-kv`` keeps the KV cache in FP8 (e4m3 codes, one f32 scale per token and KV head:
``ops/decode_attention.py``), 51.6 % of the bf16 cache's bytes (``kv_cache_mb``); the prefill quantizes its
rows in torch, which is counted in ``prefill_ms``.  It composes with the other three flags.
``--speculate K`` (1..7, greedy only, not with ``--graph`` or ``--fp8-kv``) verifies K drafted tokens per
sequence in every step (``Llama.generate(speculate=K)``, ``ops/extend_attention.py``) and adds ``spec_steps``,
``tokens_per_step`` (mean tokens a sequence emits per step) and ``ms_per_step`` to the JSON line.  The drafter is
prompt lookup over the sequence's own ids; ``--drafter oracle`` / ``wrong`` are for measurements: they draft from
the ids of a plain run made first (not timed), all right (the upper bound) or all wrong (the overhead).
``--repeat-prompt N`` makes the synthetic prompts repeat an N-token pattern, which prompt lookup can use.

The project has no tokenizer: prompts are token ids, from ``--prompt-ids FILE`` (a JSON list of id
lists, which may be ragged) or synthetic ones drawn like the training data.
"""
from __future__ import annotations

import argparse
import json
import sys
import time

import torch

from ..models.llama3 import Llama, LlamaConfig
from ..ops.decode_attention import kv_cache_bytes
from ..parallel.flat import FlatParamStore


def load_checkpoint_params(model: Llama, path: str, bucket_mb: float = 256.0) -> None:
    """Fill ``model``'s parameters from the ``param_buf`` of a checkpoint written by ``Trainer.save``.

    The flat layout is :meth:`FlatParamStore.param_layout` -- the store's own code -- so no gradient
    or optimizer buffer is allocated.  ``bucket_mb`` only matters for a checkpoint of a sharded
    (ZeRO-1) run, whose buckets are padded per rank: pass the training run's value."""
    st = torch.load(path, map_location="cpu", weights_only=True)
    zero_world = int(st.get("zero_world", torch.tensor(0)))
    names, params, offs, numel = FlatParamStore.param_layout(
        model.params_in_backward_order(), dtype=st["param_buf"].dtype, bucket_mb=bucket_mb,
        world=max(1, zero_world), sharded=zero_world > 0)
    if st["names"] != "\n".join(names):
        raise ValueError("checkpoint does not match this model's parameter layout")
    buf = st["param_buf"]
    if buf.numel() != numel:
        raise ValueError(f"checkpoint holds {buf.numel()} flat elements, this model's layout has {numel} "
                         "(a sharded run's --bucket-mb must be given)")
    with torch.no_grad():
        for p, o in zip(params, offs):
            p.copy_(buf[o: o + p.numel()].view(p.shape))


def _prompts(args, cfg: LlamaConfig, device: torch.device) -> tuple[torch.Tensor, list[int]]:
    if args.prompt_ids:
        with open(args.prompt_ids) as f:
            rows = json.load(f)
        if not rows or not all(isinstance(r, list) and r for r in rows):
            raise ValueError("--prompt-ids: expected a JSON list of non-empty id lists")
        if any(not 0 <= int(t) < cfg.vocab_size for r in rows for t in r):
            raise ValueError(f"--prompt-ids: ids must be in [0, {cfg.vocab_size})")
        lens = [len(r) for r in rows]
        tokens = torch.zeros((len(rows), max(lens)), dtype=torch.long)
        for b, r in enumerate(rows):
            tokens[b, : len(r)] = torch.tensor(r, dtype=torch.long)
        return tokens.to(device), lens
    gen = torch.Generator(device=device)
    gen.manual_seed(args.seed)
    if args.repeat_prompt:
        pattern = torch.randint(0, cfg.vocab_size, (args.batch, args.repeat_prompt), device=device, generator=gen)
        tokens = pattern.repeat(1, -(-args.prompt_len // args.repeat_prompt))[:, : args.prompt_len].contiguous()
    else:
        tokens = torch.randint(0, cfg.vocab_size, (args.batch, args.prompt_len), device=device, generator=gen)
    return tokens, [args.prompt_len] * args.batch


def _reference_drafter(ids: list[list[int]], lens: list[int], vocab: int, right: bool):
    """A measurement ``draft_fn`` from the ids of a plain run: every draft right, or every draft wrong."""
    def draft(histories, k):
        out = []
        for b, h in enumerate(histories):
            e = len(h) - lens[b]
            true = (ids[b] + [0] * k)[e: e + k]
            out.append(true if right else [(t + 1) % vocab for t in true])
        return out

    return draft


def main(argv: list[str] | None = None) -> int:
    ap = argparse.ArgumentParser(description="Llama-3 bf16 generation on MI355X (KV cache, split-KV decode)")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--ckpt", default=None, help="checkpoint written by the training payload (default: random init)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt-len", type=int, default=512)
    ap.add_argument("--prompt-ids", default=None, help="JSON file: a list of token-id lists (may be ragged)")
    ap.add_argument("--max-new-tokens", type=int, default=64)
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--top-k", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log-every", type=int, default=8)
    ap.add_argument("--device", default=None, help="default: cuda when available, else cpu")
    ap.add_argument("--stream-gemm", action="store_true",
                    help="decode steps run their GEMMs on the weight-streaming kernel (ops/decode_linear.py)")
    ap.add_argument("--graph", action="store_true",
                    help="capture the decode step into a graph and replay it per token (models/decode_graph.py)")
    ap.add_argument("--fp8-weights", action="store_true",
                    help="decode steps run on FP8 (e4m3, per-row scale) copies of the weights "
                         "(ops/decode_linear_fp8.py); the prefill stays on bf16")
    ap.add_argument("--fp8-kv", action="store_true",
                    help="keep the KV cache as FP8 (e4m3) codes with one scale per (token, KV head) row "
                         "(ops/decode_attention.py, csrc/decode_attn_fp8.hip)")
    ap.add_argument("--speculate", type=int, default=0, metavar="K",
                    help="speculative greedy decoding: verify K (1..7) drafted tokens per sequence and step "
                         "(ops/extend_attention.py); not with --graph, --fp8-kv or a temperature")
    ap.add_argument("--drafter", choices=("lookup", "oracle", "wrong"), default="lookup",
                    help="lookup: prompt lookup (default); oracle / wrong: drafts from a plain run made first, "
                         "all right / all wrong (measurements)")
    ap.add_argument("--repeat-prompt", type=int, default=0, metavar="N",
                    help="synthetic prompts repeat an N-token pattern")
    args = ap.parse_args(argv)
    from ..utils.blas_env import refuse_unsafe_blas_workspace

    refuse_unsafe_blas_workspace("th-gen")
    device = torch.device(args.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    cfg = LlamaConfig.named(args.model)
    model = Llama(cfg, device=device, dtype=torch.bfloat16, seed=args.seed)
    if args.ckpt:
        load_checkpoint_params(model, args.ckpt)
    tokens, lens = _prompts(args, cfg, device)
    batch = tokens.shape[0]
    sampler = torch.Generator(device=device)
    sampler.manual_seed(args.seed + 1)

    def sync() -> float:
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        return time.perf_counter()

    quantize_ms = None
    if args.fp8_weights:
        t = sync()
        model.quantize_decode_weights()
        quantize_ms = round(1000.0 * (sync() - t), 3)
    marks = {"t0": sync(), "last": None, "last_step": 0}

    def on_step(i: int) -> None:
        if i == 0:
            marks["prefill"] = marks["last"] = sync()
        elif args.speculate:  # a step emits a varying number of tokens: the rates are printed at the end
            return
        elif i % args.log_every == 0 or i == args.max_new_tokens - 1:
            now = sync()
            tps = batch * (i - marks["last_step"]) / max(now - marks["last"], 1e-9)
            print(f"[th-gen] step={i} tokens/s={tps:.1f} batch={batch}", flush=True)
            marks["last"], marks["last_step"] = now, i

    spec_stats: dict = {}
    draft_fn = None
    if args.speculate:
        if args.drafter != "lookup":  # the plain run's ids, before any clock starts
            plain = model.generate(tokens, lens, max_new_tokens=args.max_new_tokens, stream_gemm=args.stream_gemm,
                                   fp8=args.fp8_weights)
            draft_fn = _reference_drafter(plain.tolist(), lens, cfg.vocab_size, args.drafter == "oracle")
            marks["t0"] = sync()

    ids = model.generate(tokens, lens, max_new_tokens=args.max_new_tokens, temperature=args.temperature,
                         top_k=args.top_k, generator=sampler, on_step=on_step, stream_gemm=args.stream_gemm,
                         graph=args.graph, fp8=args.fp8_weights, kv_fp8=args.fp8_kv, speculate=args.speculate,
                         draft_fn=draft_fn, spec_stats=spec_stats)
    end = sync()
    spec = {}
    if args.speculate:
        steps = spec_stats["steps"]
        per_step = (args.max_new_tokens - 1) / steps if steps else None
        ms_step = 1000.0 * (end - marks["prefill"]) / steps if steps else None
        print(f"[th-gen] speculate={args.speculate} drafter={args.drafter} steps={steps} "
              f"tokens/step={per_step and round(per_step, 3)} ms/step={ms_step and round(ms_step, 3)} "
              f"accepted={spec_stats['accepted']}/{spec_stats['drafted']}", flush=True)
        spec = {"speculate": args.speculate, "drafter": args.drafter, "spec_steps": steps,
                "tokens_per_step": per_step and round(per_step, 3), "ms_per_step": ms_step and round(ms_step, 3),
                "drafts_accepted": spec_stats["accepted"], "drafts": spec_stats["drafted"]}
    decode_steps = args.max_new_tokens - 1
    kv_dtype = torch.float8_e4m3fn if args.fp8_kv else torch.bfloat16
    kv_bytes = kv_cache_bytes(cfg, batch, max(lens) + args.max_new_tokens + args.speculate, kv_dtype)  # generate()'s cache
    print(json.dumps({"event": "done", "new_tokens": int(ids.numel()),
                      "prefill_ms": round(1000.0 * (marks["prefill"] - marks["t0"]), 3),
                      "decode_ms_per_token": round(1000.0 * (end - marks["prefill"]) / decode_steps, 3)
                      if decode_steps else None, "stream_gemm": bool(args.stream_gemm),
                      "graph": bool(args.graph), "fp8_weights": bool(args.fp8_weights),
                      "quantize_ms": quantize_ms, "kv_dtype": str(kv_dtype).replace("torch.", ""),
                      "kv_cache_mb": round(kv_bytes / 2 ** 20, 1), **spec}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
