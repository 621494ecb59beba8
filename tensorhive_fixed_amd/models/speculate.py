"""Drafters for ``Llama.generate(speculate=k)``: plain Python on the host over token-id lists.

A drafter is ``draft_fn(histories, k) -> k ids per sequence``, where ``histories[b]`` holds the prompt
and every token emitted so far of sequence ``b``.  The drafts only decide how many tokens a step emits,
never which: the verification step keeps a draft only where the model's own argmax agrees.
"""
from __future__ import annotations

MAX_NGRAM = 3


def prompt_lookup(history: list[int], k: int, max_ngram: int = MAX_NGRAM) -> list[int]:
    """Prompt lookup: take the longest suffix n-gram of ``history`` (n = ``max_ngram`` .. 1) that also
    occurs earlier in it and propose the ``k`` tokens that followed its most recent earlier occurrence.
    Where fewer than ``k`` follow, the last proposed token is repeated; a history with no repeat at all
    proposes its own last token ``k`` times."""
    n_hist = len(history)
    for n in range(min(max_ngram, n_hist - 1), 0, -1):
        suffix = history[n_hist - n:]
        for i in range(n_hist - n - 1, -1, -1):  # most recent first; at least one token follows
            if history[i: i + n] == suffix:
                out = history[i + n: i + n + k]
                return out + [out[-1]] * (k - len(out))
    return [history[-1]] * k


def prompt_lookup_draft(histories: list[list[int]], k: int) -> list[list[int]]:
    """The default ``draft_fn``: ``prompt_lookup`` on every sequence's own ids."""
    return [prompt_lookup(h, k) for h in histories]
