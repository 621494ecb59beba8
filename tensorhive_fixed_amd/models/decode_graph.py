"""A decode step of :class:`~.llama3.Llama` captured once and replayed as one graph launch per token.

An eager ``decode_step`` issues about nine launches per layer from Python, each with a fresh
``torch.empty``; at batch 8 the host cannot issue them as fast as the GPU finishes them.
``DecodeGraph`` captures the body of the step (embedding to f32 logits, ``cache.lens_dev += 1``
included) on a side stream as one linear chain and replays it.  Nothing in the captured launches
depends on the current lengths: RoPE + append and the attention read ``cache.lens_dev`` on the
device, and the attention derives its split geometry there too (``decode_attention(...,
device_geometry=True)``), under a grid sized for ``cache.max_len``.  Its partials are those of the
host rule, so a replayed step has the bits of the eager step wherever the GEMMs are the project's own
kernels (``stream_gemm``, or ``fp8``: the step on FP8 weights, where all of them are).

The graph reads the cache, ``lens_dev`` and the weights through fixed addresses, so it stays valid
after ``cache.set_lens`` or another ``prefill`` into the same cache; the weights must not be
reallocated while it lives.  The object holds a reference to everything it captured, the attention
workspace included.  Sampling stays outside the graph.

On CPU tensors there is nothing to capture: the same interface runs the eager step.
"""
from __future__ import annotations

import torch

from ..ops import _lib
from ..ops.decode_attention import KVCache


class DecodeGraph:
    """``step(tokens [B]) -> logits [B, vocab] f32`` on top of ``cache``; built by ``Llama.decode_graph``."""

    def __init__(self, model, cache: KVCache, stream_gemm: bool = False, fp8: bool = False):
        model._need_add_norm("decode_graph")
        if cache.cfg != model.cfg:
            raise ValueError("decode_graph: the cache was built for another model configuration")
        if cache.kv.device != model.tok_emb.device:
            raise ValueError(f"decode_graph: the cache is on {cache.kv.device}, the model on {model.tok_emb.device}")
        if max(cache.lens) >= cache.max_len:
            raise ValueError(f"decode_graph: the cache is full ({max(cache.lens)} of {cache.max_len} rows): "
                             "no dead row to warm up on")
        self.model, self.cache, self.stream_gemm, self.fp8 = model, cache, bool(stream_gemm), bool(fp8)
        if self.fp8:  # takes precedence, as in decode_step; the FP8 weights must not be re-quantized while it lives
            model._need_fp8(cache.batch)
            self._body = model._decode_step_fp8
        else:
            self._body = model._decode_step_stream if self.stream_gemm else model._decode_step_plain
        self._graph = None
        if cache.device.type == "cuda":
            self._capture()

    def _capture(self) -> None:
        cache, dev = self.cache, self.cache.kv.device
        tun = torch.cuda.tunable
        if tun.is_enabled() and tun.tuning_is_enabled():
            raise RuntimeError("decode_graph: TunableOp tuning would time GEMMs inside the capture: use a "
                               "lookup-only table (ops/tuned) or disable it")
        _lib.load()
        self._tokens = torch.zeros(cache.batch, device=dev, dtype=torch.long)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            # once eagerly on the capture stream: BLAS handles and workspaces, the rope tables, the kernel
            # modules and the attention workspace come into being outside the capture.  K/V of token 0 go
            # to row lens[b], which is dead; the lengths do not move.
            self._body(self._tokens, cache, device_geometry=True, advance=lambda: None)
        self._workspace = cache.workspace(0)  # the buffer the captured attention launches point at
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            self._logits = self._body(self._tokens, cache, device_geometry=True,
                                      advance=lambda: cache.lens_dev.add_(1))
        self._graph = graph

    def step(self, tokens: torch.Tensor) -> torch.Tensor:
        """One new token per sequence -> f32 logits ``[B, vocab]``; advances the cache lengths by one.
        On the GPU the result is a static tensor that the next ``step`` overwrites: use or copy it
        before then.  Raises ``ValueError``, with nothing launched or changed, when the cache is full."""
        cache = self.cache
        if tokens.dim() != 1 or tokens.shape[0] != cache.batch:
            raise ValueError(f"DecodeGraph.step: expected {cache.batch} token ids, got shape {tuple(tokens.shape)}")
        if max(cache.lens) + 1 > cache.max_len:
            raise ValueError(f"DecodeGraph.step: {max(cache.lens)} + 1 rows exceed the cache's max_len "
                             f"{cache.max_len}")
        if self._graph is None:
            return self.model.decode_step(tokens, cache, stream_gemm=self.stream_gemm, fp8=self.fp8)
        self._tokens.copy_(tokens)
        self._graph.replay()
        cache.advance_host(1)  # the replay advanced lens_dev
        return self._logits
