"""Llama-3 decoder (8B configuration by default) built on the gfx950 kernels of ``ops/``.

This is the N07 payload model of SURVEY §2.12 (the reference has no model code at all; it only
*launches* user trainings -- ``examples/PyTorch/README.md:30-64``).  Architecture facts:
L = 32, d = 4096, 32 query / 8 kv heads of 128, FFN 14336 (SwiGLU), vocab 128256,
RoPE theta = 5e5, RMSNorm eps = 1e-5, untied LM head.

Per block the data flow is chosen for MI355X:
  x -> RMSNorm (HIP) -> ONE fused QKV GEMM [4096 -> 6144] -> RoPE in place + causal GQA flash
  attention straight out of the packed qkv buffer (HIP, MFMA) -> O-proj GEMM -> residual add
  fused INTO the next RMSNorm (``rmsnorm_add_fork``: one kernel reads the projection and the
  residual stream, writes their bf16 sum and the normalised row) -> ONE fused gate|up GEMM
  [4096 -> 28672] -> SwiGLU (HIP) -> down GEMM, whose residual add is again taken by the next
  block's (or the final) RMSNorm.  ``TH_ADD_NORM=0`` selects the older flow, where the O-proj and
  down GEMMs add the residual in an ``addmm`` beta = 1 epilogue; both flows are checked against
  each other in ``tests/test_rmsnorm_add.py``.
The LM head is fused with the cross-entropy (chunked, logits never materialised whole).
Every weight gradient is written by its producing GEMM/kernel into the flat DDP buffer.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass

import torch
from torch import nn

from ..ops.attention import qkv_attention
from ..ops.cross_entropy import linear_cross_entropy
from ..ops.decode_attention import KVCache, decode_attention, rope_append
from ..ops.decode_linear import decode_gate_up_swiglu, decode_linear
from ..ops.decode_linear import preferred as dl_preferred
from ..ops.decode_linear_fp8 import decode_gate_up_swiglu_fp8, decode_linear_fp8, quantize_weight_fp8, supported_fp8
from ..ops.embedding import embedding
from ..ops.extend_attention import extend_attention, rope_append_block
from ..ops.linear import linear
from ..ops.mlp import gate_up_swiglu
from ..ops.rmsnorm import rmsnorm, rmsnorm_add_fork, rmsnorm_fork
from ..ops.swiglu import swiglu


@dataclass
class LlamaConfig:
    vocab_size: int = 128256
    dim: int = 4096
    n_layers: int = 32
    n_heads: int = 32
    n_kv_heads: int = 8
    ffn_dim: int = 14336
    rope_theta: float = 500000.0
    norm_eps: float = 1e-5
    max_seq_len: int = 8192
    ce_chunk: int = 4096

    @property
    def head_dim(self) -> int:
        return self.dim // self.n_heads

    @classmethod
    def llama3_8b(cls) -> "LlamaConfig":
        # TH_CE_CHUNK: tokens per LM-head + cross-entropy chunk (logits of one chunk: chunk x 128256 bf16)
        return cls(ce_chunk=int(os.environ.get("TH_CE_CHUNK", "4096")))

    @classmethod
    def tiny(cls) -> "LlamaConfig":
        """Test-size model with the same head geometry (head_dim 128, GQA 4:1)."""
        return cls(vocab_size=512, dim=256, n_layers=2, n_heads=2, n_kv_heads=1, ffn_dim=512,
                   max_seq_len=512, ce_chunk=64)

    @classmethod
    def named(cls, name: str) -> "LlamaConfig":
        table = {"llama3-8b": cls.llama3_8b, "llama3_8b": cls.llama3_8b, "tiny": cls.tiny,
                 "llama3-1b-shape": lambda: cls(dim=2048, n_layers=16, n_heads=16, n_kv_heads=4,
                                                ffn_dim=8192)}
        return table[name.lower()]()

    def num_params(self) -> int:
        d, f, v, L = self.dim, self.ffn_dim, self.vocab_size, self.n_layers
        kv = self.n_kv_heads * self.head_dim
        per_layer = d * (d + 2 * kv) + d * d + 2 * f * d + f * d + 2 * d
        return v * d * 2 + L * per_layer + d

    def flops_per_token(self, seq_len: int) -> float:
        """Training FLOPs per token (fwd + bwd = 3x fwd), causal attention counted at half."""
        n_mat = self.num_params() - self.vocab_size * self.dim  # embedding is a gather
        attn = 2 * 2 * self.n_layers * seq_len * self.dim / 2  # QK^T + PV, causal half
        return 6 * n_mat + 3 * attn


# projections whose weight grad runs on transposed operand copies (ops/linear.py): where the GEMM
# speed-up outweighs the transposes (measured: profiles/r01_gemm/)
WGRAD_NT = set(filter(None, os.environ.get("TH_WGRAD_NT_LAYERS", "w13").split(",")))
# projections whose weight grad runs on the gfx950 TN kernel (ops/gemm_tn.py), measured faster than
# hipBLASLt there (scripts/bench_gemm_tn.py)
WGRAD_TN = set(filter(None, os.environ.get("TH_WGRAD_TN_LAYERS", "wqkv,wo,w2").split(",")))
_FORK = os.environ.get("TH_RMSNORM_FORK", "1") == "1"


# residual adds fused into the following RMSNorm (rmsnorm_add_fork) instead of beta=1 GEMM epilogues
ADD_NORM = _FORK and os.environ.get("TH_ADD_NORM", "1") == "1"


def _norm(x, w, eps):
    if _FORK:
        return rmsnorm_fork(x, w, eps)
    return rmsnorm(x, w, eps), x


class LlamaBlock(nn.Module):
    def __init__(self, cfg: LlamaConfig, device, dtype):
        super().__init__()
        d, hd = cfg.dim, cfg.head_dim
        qkv_out = (cfg.n_heads + 2 * cfg.n_kv_heads) * hd
        self.cfg = cfg
        self.attn_norm = nn.Parameter(torch.ones(d, device=device, dtype=dtype))
        self.wqkv = nn.Parameter(torch.empty(qkv_out, d, device=device, dtype=dtype))
        self.wo = nn.Parameter(torch.empty(d, cfg.n_heads * hd, device=device, dtype=dtype))
        self.ffn_norm = nn.Parameter(torch.ones(d, device=device, dtype=dtype))
        self.w13 = nn.Parameter(torch.empty(2 * cfg.ffn_dim, d, device=device, dtype=dtype))
        self.w2 = nn.Parameter(torch.empty(d, cfg.ffn_dim, device=device, dtype=dtype))

    def forward(self, x: torch.Tensor, B: int, S: int, pending: torch.Tensor | None = None):
        """Without ADD_NORM: returns the block output.  With it: returns ``(y, x)``, the MLP-down
        projection and the residual stream, whose sum the next norm forms (``pending`` of the next
        block / the final norm)."""
        c = self.cfg
        # rmsnorm_fork: the residual gradient is added inside the RMSNorm backward kernel
        if pending is not None:
            h, x = rmsnorm_add_fork(pending, x, self.attn_norm, c.norm_eps)
        else:
            h, x = _norm(x, self.attn_norm, c.norm_eps)
        qkv = linear(h, self.wqkv, wgrad_nt="wqkv" in WGRAD_NT, wgrad_tn="wqkv" in WGRAD_TN)
        o = qkv_attention(qkv, B, S, c.n_heads, c.n_kv_heads, c.head_dim, c.rope_theta)
        if ADD_NORM:
            y = linear(o, self.wo, wgrad_nt="wo" in WGRAD_NT, wgrad_tn="wo" in WGRAD_TN)
            h, x = rmsnorm_add_fork(y, x, self.ffn_norm, c.norm_eps)
        else:
            x = linear(o, self.wo, residual=x, wgrad_nt="wo" in WGRAD_NT, wgrad_tn="wo" in WGRAD_TN)
            h, x = _norm(x, self.ffn_norm, c.norm_eps)
        if "w13" in WGRAD_NT:  # fused gate|up + SwiGLU node: transposed dGU from the SwiGLU kernel
            a = gate_up_swiglu(h, self.w13)
        else:
            a = swiglu(linear(h, self.w13))
        if ADD_NORM:
            return linear(a, self.w2, wgrad_nt="w2" in WGRAD_NT, wgrad_tn="w2" in WGRAD_TN), x
        return linear(a, self.w2, residual=x, wgrad_nt="w2" in WGRAD_NT, wgrad_tn="w2" in WGRAD_TN)


class Llama(nn.Module):
    def __init__(self, cfg: LlamaConfig, device="cpu", dtype=torch.bfloat16, seed: int = 0):
        super().__init__()
        self.cfg = cfg
        self.tok_emb = nn.Parameter(torch.empty(cfg.vocab_size, cfg.dim, device=device, dtype=dtype))
        self.layers = nn.ModuleList([LlamaBlock(cfg, device, dtype) for _ in range(cfg.n_layers)])
        self.norm = nn.Parameter(torch.ones(cfg.dim, device=device, dtype=dtype))
        self.lm_head = nn.Parameter(torch.empty(cfg.vocab_size, cfg.dim, device=device, dtype=dtype))
        # ZeRO-1 hook: called with the parameters about to be read, so a sharded store can make the
        # stream wait for exactly the all-gather buckets holding them (parallel/flat.py)
        self.param_gate = None
        # (wq, scale) pairs of the decode-step weights, built by quantize_decode_weights(); a plain
        # attribute holding plain tensors: no Parameter, no buffer, invisible to state_dict()
        self.fp8_weights = None
        self.reset_parameters(seed)

    @torch.no_grad()
    def reset_parameters(self, seed: int = 0) -> None:
        g = torch.Generator(device=self.tok_emb.device)
        g.manual_seed(seed)
        std = 0.02
        out_std = std / math.sqrt(2 * self.cfg.n_layers)
        self.tok_emb.normal_(0, std, generator=g)
        self.lm_head.normal_(0, std, generator=g)
        for blk in self.layers:
            blk.wqkv.normal_(0, std, generator=g)
            blk.w13.normal_(0, std, generator=g)
            blk.wo.normal_(0, out_std, generator=g)
            blk.w2.normal_(0, out_std, generator=g)

    def params_in_backward_order(self) -> list[tuple[str, nn.Parameter, bool]]:
        """(name, param, weight_decay?) in the order backward produces their gradients."""
        out = [("lm_head", self.lm_head, True), ("norm", self.norm, False)]
        for i in reversed(range(len(self.layers))):
            b = self.layers[i]
            out += [(f"layers.{i}.w2", b.w2, True), (f"layers.{i}.w13", b.w13, True),
                    (f"layers.{i}.ffn_norm", b.ffn_norm, False), (f"layers.{i}.wo", b.wo, True),
                    (f"layers.{i}.wqkv", b.wqkv, True), (f"layers.{i}.attn_norm", b.attn_norm, False)]
        out.append(("tok_emb", self.tok_emb, True))
        return out

    def hidden(self, tokens: torch.Tensor) -> torch.Tensor:
        B, S = tokens.shape
        gate = self.param_gate
        if gate is not None:
            gate(self.tok_emb)
        x = embedding(tokens, self.tok_emb).view(B * S, self.cfg.dim)
        pending = None
        for blk in self.layers:
            if gate is not None:
                gate(blk.attn_norm, blk.wqkv, blk.wo, blk.ffn_norm, blk.w13, blk.w2)
            if ADD_NORM:
                pending, x = blk(x, B, S, pending)
            else:
                x = blk(x, B, S)
        if gate is not None:
            gate(self.norm, self.lm_head)
        if pending is not None:
            return rmsnorm_add_fork(pending, x, self.norm, self.cfg.norm_eps)[0]
        return rmsnorm(x, self.norm, self.cfg.norm_eps)

    def forward(self, tokens: torch.Tensor, targets: torch.Tensor | None = None,
                n_valid: int | None = None) -> torch.Tensor:
        """Returns the mean CE loss when ``targets`` is given, else the final hidden states."""
        h = self.hidden(tokens)
        if targets is None:
            return h
        return linear_cross_entropy(h, self.lm_head, targets.reshape(-1), self.cfg.ce_chunk,
                                    n_valid=n_valid)

    @torch.no_grad()
    def logits(self, tokens: torch.Tensor) -> torch.Tensor:
        return torch.mm(self.hidden(tokens), self.lm_head.t()).view(*tokens.shape, -1)

    # ------------------------------------------------------------------ generation (KV cache)
    @staticmethod
    def _need_add_norm(what: str) -> None:
        if not ADD_NORM:
            raise RuntimeError(f"Llama.{what} runs the fused add+norm flow only: unset TH_ADD_NORM=0 / "
                               "TH_RMSNORM_FORK=0")

    @torch.no_grad()
    def prefill(self, tokens: torch.Tensor, prompt_lens, cache: KVCache) -> torch.Tensor:
        """Run the left-aligned prompts ``tokens [B, S]`` through the training forward (flash attention,
        RoPE in place on the packed qkv), store every layer's rotated K and its V in ``cache``
        (``KVCache.fill``: a copy, or the quantization of an FP8 cache) and set
        the cache lengths to ``prompt_lens``.  Returns the final-norm hidden state ``[B, dim]`` at
        position ``prompt_lens[b] - 1``.  Padding after a prompt is masked out of every real position
        by causality; its cache rows are dead by the lengths."""
        self._need_add_norm("prefill")
        c = self.cfg
        B, S = tokens.shape
        lens = [int(n) for n in prompt_lens]
        if B != cache.batch or len(lens) != B or min(lens) < 1 or max(lens) > S or S > cache.max_len:
            raise ValueError(f"prefill: prompts {lens} in a [{B}, {S}] batch do not fit the cache "
                             f"(batch {cache.batch}, max_len {cache.max_len})")
        Hq, Hkv, Dh = c.n_heads, c.n_kv_heads, c.head_dim
        x = embedding(tokens, self.tok_emb).view(B * S, c.dim)
        pending = None
        for i, blk in enumerate(self.layers):
            if pending is None:
                h, x = _norm(x, blk.attn_norm, c.norm_eps)
            else:
                h, x = rmsnorm_add_fork(pending, x, blk.attn_norm, c.norm_eps)
            qkv = linear(h, blk.wqkv)
            o = qkv_attention(qkv, B, S, Hq, Hkv, Dh, c.rope_theta)  # rotates q / k of qkv in place
            kv = qkv.view(B, S, Hq + 2 * Hkv, Dh)
            cache.fill(i, kv[:, :, Hq: Hq + Hkv].transpose(1, 2), kv[:, :, Hq + Hkv:].transpose(1, 2))
            h, x = rmsnorm_add_fork(linear(o, blk.wo), x, blk.ffn_norm, c.norm_eps)
            pending = linear(swiglu(linear(h, blk.w13)), blk.w2)
        cache.set_lens(lens)
        rows = torch.tensor([b * S + n - 1 for b, n in enumerate(lens)], device=tokens.device)
        return rmsnorm_add_fork(pending[rows].contiguous(), x[rows].contiguous(), self.norm, c.norm_eps)[0]

    @torch.no_grad()
    def decode_step(self, tokens: torch.Tensor, cache: KVCache, stream_gemm: bool = False,
                    fp8: bool = False) -> torch.Tensor:
        """One new token per sequence (``tokens [B]``) on top of ``cache`` -> f32 logits ``[B, vocab]``;
        advances the cache lengths by one.  ``stream_gemm`` runs the projections and the LM head on the
        weight-streaming kernel of ``ops/decode_linear.py`` wherever its ``preferred`` allows.  ``fp8``
        (which takes precedence) runs all of them on the FP8 weights of ``quantize_decode_weights()``
        with ``ops/decode_linear_fp8.py``; it raises when they are missing or the batch is above 16."""
        self._need_add_norm("decode_step")
        c = self.cfg
        B = tokens.shape[0]
        if tokens.dim() != 1 or B != cache.batch:
            raise ValueError(f"decode_step: expected {cache.batch} token ids, got shape {tuple(tokens.shape)}")
        if fp8:
            return self._decode_step_fp8(tokens, cache)
        if stream_gemm:
            return self._decode_step_stream(tokens, cache)
        return self._decode_step_plain(tokens, cache)

    def _decode_step_plain(self, tokens: torch.Tensor, cache: KVCache, device_geometry: bool = False,
                           advance=None) -> torch.Tensor:
        """The body of ``decode_step`` on hipBLASLt GEMMs.  ``advance`` replaces ``cache.advance(1)``
        and ``device_geometry`` is passed to ``decode_attention``: both are what a captured step
        (``decode_graph``) changes, which must not read the host lengths or move them."""
        c = self.cfg
        B = tokens.shape[0]
        x = embedding(tokens.view(B, 1), self.tok_emb).view(B, c.dim)
        pending = None
        for i, blk in enumerate(self.layers):
            if pending is None:
                h, x = _norm(x, blk.attn_norm, c.norm_eps)
            else:
                h, x = rmsnorm_add_fork(pending, x, blk.attn_norm, c.norm_eps)
            q = rope_append(linear(h, blk.wqkv), cache, i)
            o = decode_attention(q, cache, i, new=1, device_geometry=device_geometry)
            h, x = rmsnorm_add_fork(linear(o, blk.wo), x, blk.ffn_norm, c.norm_eps)
            pending = linear(swiglu(linear(h, blk.w13)), blk.w2)
        if advance is None:
            cache.advance(1)
        else:
            advance()
        h = rmsnorm_add_fork(pending, x, self.norm, c.norm_eps)[0]
        return torch.mm(h, self.lm_head.t()).float()

    def _decode_step_stream(self, tokens: torch.Tensor, cache: KVCache, device_geometry: bool = False,
                            advance=None) -> torch.Tensor:
        """``decode_step`` with every GEMM on ``decode_linear`` where ``preferred`` allows (gate|up and
        SwiGLU in one call, f32 logits from the f32 accumulator); any other shape, such as a batch
        above 16 or one measured faster on hipBLASLt, takes the GEMM of the default path.
        ``device_geometry`` and ``advance`` as in ``_decode_step_plain``."""
        c = self.cfg
        B = tokens.shape[0]

        def proj(a, w):
            return decode_linear(a, w) if dl_preferred(B, w.shape[0], w.shape[1]) else linear(a, w)

        x = embedding(tokens.view(B, 1), self.tok_emb).view(B, c.dim)
        pending = None
        for i, blk in enumerate(self.layers):
            if pending is None:
                h, x = _norm(x, blk.attn_norm, c.norm_eps)
            else:
                h, x = rmsnorm_add_fork(pending, x, blk.attn_norm, c.norm_eps)
            q = rope_append(proj(h, blk.wqkv), cache, i)
            o = decode_attention(q, cache, i, new=1, device_geometry=device_geometry)
            h, x = rmsnorm_add_fork(proj(o, blk.wo), x, blk.ffn_norm, c.norm_eps)
            if dl_preferred(B, c.ffn_dim, c.dim):
                a = decode_gate_up_swiglu(h, blk.w13)
            else:
                a = swiglu(linear(h, blk.w13))
            pending = proj(a, blk.w2)
        if advance is None:
            cache.advance(1)
        else:
            advance()
        h = rmsnorm_add_fork(pending, x, self.norm, c.norm_eps)[0]
        if dl_preferred(B, c.vocab_size, c.dim):
            return decode_linear(h, self.lm_head, out_dtype=torch.float32)
        return torch.mm(h, self.lm_head.t()).float()

    @torch.no_grad()
    def quantize_decode_weights(self) -> None:
        """Build and keep the FP8 form (``ops/decode_linear_fp8.quantize_weight_fp8``: e4m3 codes and one
        f32 scale per output row) of every layer's ``wqkv``, ``wo``, ``w13`` and ``w2`` and of ``lm_head``,
        for ``decode_step(fp8=True)``.  The bf16 parameters stay (the prefill runs on them), so this adds
        half their bytes.  Call it again after the parameters change, e.g. after a checkpoint load: the
        FP8 copies do not follow them.  A weight shape the FP8 kernel does not take raises here."""
        ws = [(f"layers.{i}.{n}", getattr(blk, n)) for i, blk in enumerate(self.layers)
              for n in ("wqkv", "wo", "w13", "w2")] + [("lm_head", self.lm_head)]
        for name, w in ws:
            if not supported_fp8(1, w.shape[0], w.shape[1]):
                raise ValueError(f"quantize_decode_weights: {name} {tuple(w.shape)} is outside the FP8 decode "
                                 "kernel's shape rule (ops/decode_linear_fp8.supported_fp8)")
        q = {name: quantize_weight_fp8(w.detach().contiguous()) for name, w in ws}
        self.fp8_weights = {"layers": [{n: q[f"layers.{i}.{n}"] for n in ("wqkv", "wo", "w13", "w2")}
                                       for i in range(len(self.layers))], "lm_head": q["lm_head"]}

    def _need_fp8(self, B: int) -> dict:
        if self.fp8_weights is None:
            raise ValueError("decode_step(fp8=True): call quantize_decode_weights() first")
        if B > 16:
            raise ValueError(f"decode_step(fp8=True): batch {B} is above the 16 rows of the FP8 decode kernel "
                             "(there is no other FP8 path to take)")
        return self.fp8_weights

    def _decode_step_fp8(self, tokens: torch.Tensor, cache: KVCache, device_geometry: bool = False,
                         advance=None) -> torch.Tensor:
        """``decode_step`` with all five GEMMs on the FP8 weights (``ops/decode_linear_fp8.py``): gate|up
        and SwiGLU in one call, f32 logits from the f32 accumulator.  No shape falls back to the bf16
        weights, so the numerics do not depend on the batch size.  ``device_geometry`` and ``advance``
        as in ``_decode_step_plain``."""
        c = self.cfg
        B = tokens.shape[0]
        fw = self._need_fp8(B)
        x = embedding(tokens.view(B, 1), self.tok_emb).view(B, c.dim)
        pending = None
        for i, (blk, q) in enumerate(zip(self.layers, fw["layers"])):
            if pending is None:
                h, x = _norm(x, blk.attn_norm, c.norm_eps)
            else:
                h, x = rmsnorm_add_fork(pending, x, blk.attn_norm, c.norm_eps)
            qv = rope_append(decode_linear_fp8(h, *q["wqkv"]), cache, i)
            o = decode_attention(qv, cache, i, new=1, device_geometry=device_geometry)
            h, x = rmsnorm_add_fork(decode_linear_fp8(o, *q["wo"]), x, blk.ffn_norm, c.norm_eps)
            pending = decode_linear_fp8(decode_gate_up_swiglu_fp8(h, *q["w13"]), *q["w2"])
        if advance is None:
            cache.advance(1)
        else:
            advance()
        h = rmsnorm_add_fork(pending, x, self.norm, c.norm_eps)[0]
        return decode_linear_fp8(h, *fw["lm_head"], out_dtype=torch.float32)

    @torch.no_grad()
    def extend_step(self, tokens: torch.Tensor, cache: KVCache, stream_gemm: bool = False,
                    fp8: bool = False) -> torch.Tensor:
        """``T`` new tokens per sequence at once (``tokens [B, T]``, ``1 <= T <= 8``) on top of a bf16
        ``cache`` -> f32 logits ``[B, T, vocab]``; advances the cache lengths by ``T``.  It is the body of
        ``decode_step`` on ``B * T`` rows with ``rope_append_block`` / ``extend_attention``
        (``ops/extend_attention.py``) in place of the single-token ops: row ``(b, t)`` sits at position
        ``lens[b] + t`` and attends to the old rows and to the block up to itself.  ``stream_gemm`` dispatches
        on ``preferred(B * T, ...)``, so more than 16 rows take hipBLASLt; ``fp8`` raises above 16 rows."""
        self._need_add_norm("extend_step")
        c = self.cfg
        if tokens.dim() != 2 or tokens.shape[0] != cache.batch:
            raise ValueError(f"extend_step: expected token ids [{cache.batch}, T], got shape {tuple(tokens.shape)}")
        B, T = tokens.shape
        M = B * T
        fw = None
        if fp8:
            if self.fp8_weights is None:
                raise ValueError("extend_step(fp8=True): call quantize_decode_weights() first")
            if M > 16:
                raise ValueError(f"extend_step(fp8=True): {B} x {T} rows are above the 16 rows of the FP8 decode "
                                 "kernel (there is no other FP8 path to take)")
            fw = self.fp8_weights

        def proj(a, w, qw):
            if fw is not None:
                return decode_linear_fp8(a, *qw)
            if stream_gemm and dl_preferred(M, w.shape[0], w.shape[1]):
                return decode_linear(a, w)
            return linear(a, w)

        x = embedding(tokens, self.tok_emb).view(M, c.dim)
        pending = None
        for i, blk in enumerate(self.layers):
            qw = fw["layers"][i] if fw is not None else dict.fromkeys(("wqkv", "wo", "w13", "w2"))
            if pending is None:
                h, x = _norm(x, blk.attn_norm, c.norm_eps)
            else:
                h, x = rmsnorm_add_fork(pending, x, blk.attn_norm, c.norm_eps)
            q = rope_append_block(proj(h, blk.wqkv, qw["wqkv"]).view(B, T, -1), cache, i)
            o = extend_attention(q, cache, i).view(M, -1)
            h, x = rmsnorm_add_fork(proj(o, blk.wo, qw["wo"]), x, blk.ffn_norm, c.norm_eps)
            if fw is not None:
                a = decode_gate_up_swiglu_fp8(h, *qw["w13"])
            elif stream_gemm and dl_preferred(M, c.ffn_dim, c.dim):
                a = decode_gate_up_swiglu(h, blk.w13)
            else:
                a = swiglu(linear(h, blk.w13))
            pending = proj(a, blk.w2, qw["w2"])
        cache.advance(T)
        h = rmsnorm_add_fork(pending, x, self.norm, c.norm_eps)[0]
        if fw is not None:
            logits = decode_linear_fp8(h, *fw["lm_head"], out_dtype=torch.float32)
        elif stream_gemm and dl_preferred(M, c.vocab_size, c.dim):
            logits = decode_linear(h, self.lm_head, out_dtype=torch.float32)
        else:
            logits = torch.mm(h, self.lm_head.t()).float()
        return logits.view(B, T, -1)

    @torch.no_grad()
    def decode_graph(self, cache: KVCache, stream_gemm: bool = False, fp8: bool = False):
        """``decode_step`` on ``cache`` captured into a graph (``models/decode_graph.py``): the returned
        object's ``step(tokens)`` replays it with one launch per token.  On the CPU it runs the eager step."""
        from .decode_graph import DecodeGraph

        return DecodeGraph(self, cache, stream_gemm=stream_gemm, fp8=fp8)

    @staticmethod
    def sample(logits: torch.Tensor, temperature: float = 0.0, top_k: int | None = None,
               generator: torch.Generator | None = None) -> torch.Tensor:
        """Next token ids ``[B]`` from f32 logits ``[B, vocab]``: argmax at temperature 0, else a draw
        from softmax(logits / temperature) restricted to the ``top_k`` largest."""
        if temperature <= 0.0:
            return logits.argmax(-1)
        z = logits.float() / temperature
        if top_k is not None and 0 < top_k < z.shape[-1]:
            kth = z.topk(top_k, dim=-1).values[:, -1:]
            z = z.masked_fill(z < kth, float("-inf"))
        return torch.multinomial(z.softmax(-1), 1, generator=generator)[:, 0]

    @torch.no_grad()
    def generate(self, tokens: torch.Tensor, prompt_lens=None, max_new_tokens: int = 16,
                 temperature: float = 0.0, top_k: int | None = None,
                 generator: torch.Generator | None = None, return_logits: bool = False,
                 on_step=None, stream_gemm: bool = False, graph: bool = False, fp8: bool = False,
                 kv_fp8: bool = False, speculate: int = 0, draft_fn=None, spec_stats: dict | None = None):
        """Continue the left-aligned prompts ``tokens [B, S]`` (``prompt_lens`` defaults to ``S`` for all)
        by ``max_new_tokens`` tokens -> ids ``[B, max_new_tokens]`` (and the f32 logits
        ``[B, max_new_tokens, vocab]`` of every step with ``return_logits``).  ``on_step(i)`` is called
        after step ``i``'s token is chosen (step 0 comes from the prefill).  ``stream_gemm`` is passed to
        every ``decode_step``; the prefill is the same either way.  ``graph`` captures the decode step
        once after the prefill (``decode_graph``) and replays it for every further token.  ``fp8`` runs
        the decode steps on FP8 weights (``decode_step(fp8=True)``), quantizing them first if
        ``quantize_decode_weights()`` has not been called; the prefill stays on the bf16 weights.
        ``kv_fp8`` keeps the KV cache as FP8 codes with one scale per (token, KV head) row
        (``KVCache(dtype=torch.float8_e4m3fn)``): the prefill quantizes its rows into it and the decode
        steps append and attend in FP8; it composes with the other three.
        ``speculate = k`` (1..7) turns on speculative greedy decoding (``_generate_speculative``): every
        step verifies ``k`` drafted tokens per sequence in one ``extend_step``; the ids are those of the
        plain greedy run.  It needs ``temperature == 0``, ``graph=False`` and ``kv_fp8=False``.  ``draft_fn``
        replaces the prompt-lookup drafter and ``spec_stats`` receives the step counts."""
        if speculate:
            return self._generate_speculative(tokens, prompt_lens, max_new_tokens, int(speculate), draft_fn,
                                              spec_stats, temperature=temperature, graph=graph, kv_fp8=kv_fp8,
                                              return_logits=return_logits, on_step=on_step,
                                              stream_gemm=stream_gemm, fp8=fp8)
        B, S = tokens.shape
        lens = [S] * B if prompt_lens is None else [int(n) for n in prompt_lens]
        if max_new_tokens < 1:
            raise ValueError("generate: max_new_tokens must be at least 1")
        S = max(lens) if lens else S
        max_len = S + max_new_tokens  # the prefill runs at max(lens), unpadded (tests/gpu/test_flash_tails_gpu.py)
        if max_len > self.cfg.max_seq_len:
            raise ValueError(f"generate: {S} prompt + {max_new_tokens} new tokens exceed max_seq_len "
                             f"{self.cfg.max_seq_len}")
        if fp8:
            if self.fp8_weights is None:
                self.quantize_decode_weights()
            self._need_fp8(B)  # before the prefill, not after it
        cache = KVCache(self.cfg, B, max_len, tokens.device,
                        dtype=torch.float8_e4m3fn if kv_fp8 else torch.bfloat16)
        if len(lens) != B or min(lens) < 1 or S > tokens.shape[1]:
            raise ValueError(f"generate: prompt lengths {lens} do not fit tokens of shape {tuple(tokens.shape)}")
        live = torch.arange(S, device=tokens.device)[None, :] < torch.tensor(lens, device=tokens.device)[:, None]
        h = self.prefill(tokens[:, :S] * live, lens, cache)  # token 0 after every prompt
        logits = torch.mm(h, self.lm_head.t()).float()
        captured = (self.decode_graph(cache, stream_gemm=stream_gemm, fp8=fp8)
                    if graph and max_new_tokens > 1 else None)
        out, steps = [], []
        for i in range(max_new_tokens):
            if i and captured is not None:
                logits = captured.step(out[-1])
            elif i:
                logits = self.decode_step(out[-1], cache, stream_gemm=stream_gemm, fp8=fp8)
            out.append(self.sample(logits, temperature, top_k, generator))
            if return_logits:
                steps.append(logits.clone() if captured is not None else logits)  # a replay reuses its output
            if on_step is not None:
                on_step(i)
        ids = torch.stack(out, dim=1)
        return (ids, torch.stack(steps, dim=1)) if return_logits else ids

    def _generate_speculative(self, tokens, prompt_lens, max_new_tokens, k, draft_fn, spec_stats, *,
                              temperature, graph, kv_fp8, return_logits, on_step, stream_gemm, fp8):
        """``generate(speculate=k)``.  After the prefill has chosen token 0, every step feeds
        ``[last emitted token, k drafts]`` of every sequence to ``extend_step`` (T = k + 1).  Draft ``i`` is
        accepted while it equals the argmax of the logits row before it; the argmax at the first mismatch
        (after the last draft, if all match) is emitted as well, so a sequence emits 1..k+1 tokens per step,
        never more than it still needs.  ``set_lens`` then moves every cache length by what its sequence
        emitted, which leaves the rejected rows dead.  The ids go to the host once per step (one sync):
        the acceptance and the drafter (``draft_fn(histories, k) -> k ids per sequence``, default
        ``speculate.prompt_lookup_draft`` over prompt + emitted ids) run there.  ``on_step(0)`` follows the
        prefill and ``on_step(n)`` the n-th verification step.  ``spec_stats`` receives ``steps``,
        ``drafted``, ``accepted`` (drafts that were emitted), per-sequence ``emitted`` and ``cache_lens``."""
        from .speculate import prompt_lookup_draft

        if not 1 <= k <= 7:
            raise ValueError(f"generate: speculate must be in [1, 7] (a block holds at most 8 tokens), got {k}")
        if temperature != 0:
            raise ValueError("generate: speculate verifies greedy tokens only, it needs temperature == 0")
        if graph:
            raise ValueError("generate: speculate does not run on a captured step (graph=True)")
        if kv_fp8:
            raise ValueError("generate: speculate needs a bf16 KV cache (kv_fp8=True): block steps have no FP8 kernel")
        if max_new_tokens < 1:
            raise ValueError("generate: max_new_tokens must be at least 1")
        B, S = tokens.shape
        lens = [S] * B if prompt_lens is None else [int(n) for n in prompt_lens]
        S = max(lens) if lens else S
        max_len = S + max_new_tokens + k  # the last step of a sequence may append k rows it does not keep
        if max_len > self.cfg.max_seq_len:
            raise ValueError(f"generate: {S} prompt + {max_new_tokens} new + {k} draft tokens exceed max_seq_len "
                             f"{self.cfg.max_seq_len}")
        if len(lens) != B or min(lens) < 1 or S > tokens.shape[1]:
            raise ValueError(f"generate: prompt lengths {lens} do not fit tokens of shape {tuple(tokens.shape)}")
        if fp8:
            if self.fp8_weights is None:
                self.quantize_decode_weights()
            if B * (k + 1) > 16:
                raise ValueError(f"generate: fp8 with speculate={k} makes {B} x {k + 1} rows per step, above the "
                                 "16 rows of the FP8 decode kernel")
        draft = draft_fn if draft_fn is not None else prompt_lookup_draft
        cache = KVCache(self.cfg, B, max_len, tokens.device)
        live = torch.arange(S, device=tokens.device)[None, :] < torch.tensor(lens, device=tokens.device)[:, None]
        h = self.prefill(tokens[:, :S] * live, lens, cache)
        logits = torch.mm(h, self.lm_head.t()).float()
        first = logits.argmax(-1).tolist()
        hist = [row[:n] + [t] for row, n, t in zip(tokens.tolist(), lens, first)]  # prompt + emitted
        emitted = [1] * B
        rows = [[logits[b]] for b in range(B)] if return_logits else None
        if on_step is not None:
            on_step(0)
        stats = {"steps": 0, "drafted": 0, "accepted": 0}
        while min(emitted) < max_new_tokens:
            drafts = [[int(t) for t in d] for d in draft([list(x) for x in hist], k)]
            if len(drafts) != B or any(len(d) != k for d in drafts):
                raise ValueError(f"generate: draft_fn must return {k} ids for each of the {B} sequences")
            block = torch.tensor([[x[-1]] + d for x, d in zip(hist, drafts)], dtype=tokens.dtype,
                                 device=tokens.device)
            before = list(cache.lens)
            logits = self.extend_step(block, cache, stream_gemm=stream_gemm, fp8=fp8)
            pred = logits.argmax(-1).tolist()  # the step's one sync
            after = []
            for b in range(B):
                need = max_new_tokens - emitted[b]
                if need == 0:  # a finished sequence rides along: its length stays, its rows are dead
                    after.append(before[b])
                    continue
                match = 0
                while match < k and drafts[b][match] == pred[b][match]:
                    match += 1
                a = min(match + 1, need)
                hist[b] += pred[b][:a]
                emitted[b] += a
                after.append(before[b] + a)
                stats["drafted"] += k
                stats["accepted"] += min(match, a)
                if rows is not None:
                    rows[b] += list(logits[b, :a])
            cache.set_lens(after)
            stats["steps"] += 1
            if on_step is not None:
                on_step(stats["steps"])
        if spec_stats is not None:
            spec_stats.update(stats, emitted=list(emitted), cache_lens=list(cache.lens))
        ids = torch.tensor([x[n:] for x, n in zip(hist, lens)], dtype=torch.long, device=tokens.device)
        if return_logits:
            return ids, torch.stack([torch.stack(r) for r in rows])
        return ids
