"""The ``nsplit`` argument of ``chunk_attention`` on the CPU, the rule ``pick_chunk_nsplit`` and the build
flags of the kernel file."""
import pytest
import torch

from tensorhive_fixed_amd.ops.chunk_attention import (MAX_CHUNK_SPLITS, MIN_KEYS_PER_CHUNK_SPLIT, chunk_attention,
                                                      chunk_attention_reference, pick_chunk_nsplit)
from tensorhive_fixed_amd.ops.decode_attention import KVCache
from tests.decode_oracles import attn_cfg


def test_nsplit_argument():
    cache = KVCache(attn_cfg(4, 2), 2, 16)
    cache.kv.normal_()
    cache.set_lens([3, 10])
    q = torch.randn(2, 5, 4 * 128).bfloat16()
    ref = chunk_attention_reference(q, cache, 0, [5, 2])
    for n in range(1, MAX_CHUNK_SPLITS + 1):
        assert torch.equal(chunk_attention(q, cache, 0, [5, 2], nsplit=n), ref)
    for bad in (0, MAX_CHUNK_SPLITS + 1):
        with pytest.raises(ValueError, match="chunk_attention"):
            chunk_attention(q, cache, 0, [5, 2], nsplit=bad)


def test_the_build_finds_the_kernel_files_flags():
    from tensorhive_fixed_amd.ops import build

    assert "-fno-slp-vectorize" in build.source_flags(build.CSRC / "chunk_attn.hip")  # read from 40 lines only


def test_pick_chunk_nsplit():
    assert MAX_CHUNK_SPLITS == 16 and MIN_KEYS_PER_CHUNK_SPLIT >= 1024
    # at most 1024 keys: never split, whatever the grid
    assert all(pick_chunk_nsplit(b, h, rep, T, keys, 256) == 1 for b in (1, 3, 8) for h in (1, 2, 8)
               for rep in (1, 2, 4, 8) for T in (1, 9, 129, 1024) for keys in (1, 1023, 1024))
    assert pick_chunk_nsplit(1, 8, 4, 512, 4096, 256) == 2
    assert pick_chunk_nsplit(1, 1, 4, 32, 1 << 20, 256) == MAX_CHUNK_SPLITS  # the cap
    assert pick_chunk_nsplit(1, 1, 4, 32, 3 * MIN_KEYS_PER_CHUNK_SPLIT + 5, 256) == 3  # keys per split
    assert pick_chunk_nsplit(8, 8, 4, 512, 8192, 256) == 1  # 1024 workgroups unsplit
    assert pick_chunk_nsplit(1, 8, 4, 1024, 8192, 256) == 1  # exactly n_cus workgroups
