"""What the one-call searches of capnet.ops share, as far as it runs without a device: the splitter of the packed result
buffer (seqs int64 [n, SL] | lengths int32 [n] | the error word, in n SL + n // 2 + 1 int64 words) on hand-built host
tensors, and the key of the workspace cache on a stub size function."""
import types

import pytest
import torch

from capnet import ops
from capnet._lib import CapnetError

SL = 3


def _packed(rows, lens, word):
    n = len(rows)
    host = torch.full((n * SL + n // 2 + 1,), -7, dtype=torch.int64)
    host[:n * SL] = torch.tensor(rows, dtype=torch.int64).reshape(-1)
    tail = host[n * SL:].view(torch.int32)
    assert tail.numel() in (n + 1, n + 2)              # odd n: the error word fills the last int64; even n: one word spare
    tail[:n] = torch.tensor(lens, dtype=torch.int32)
    tail[n] = word
    return host


@pytest.mark.parametrize("word", [0, 2, 1 << 20])
@pytest.mark.parametrize("lens", [(1,), (SL,), (1, SL), (SL, 1), (2, 1, SL), (SL, SL, 1), (1, 2, SL, 1), (SL, 1, 1, SL)], ids=str)
def test_the_packed_result_splits_into_lists_lengths_and_the_error_word(lens, word):
    n = len(lens)
    rows = [[10 * i + 1, 10 * i + 2, 10 * i + 3] for i in range(n)]
    lists, got, w = ops.split_result(_packed(rows, lens, word), n)
    assert lists == [rows[i][:lens[i]] for i in range(n)]
    assert got == list(lens) and all(isinstance(x, int) for x in got)
    assert w == word and isinstance(w, int)


def test_the_result_buffer_has_the_size_the_splitter_reads():
    for n in (1, 2, 3, 4):
        packed, seqs, lengths = ops._result_buffer(n, SL - 2, "cpu")
        assert packed.dtype == torch.int64 and packed.numel() == n * SL + n // 2 + 1
        assert seqs.value == packed.data_ptr() and lengths.value == packed.data_ptr() + 8 * n * SL
        packed.zero_()
        assert ops.split_result(packed, n) == ([[]] * n, [0] * n, 0)


def test_the_workspace_cache_is_keyed_by_size_function_device_and_dims(monkeypatch):
    calls = []

    def size_fn(name, nbytes):
        return lambda *dims: calls.append((name, dims)) or nbytes
    stub = types.SimpleNamespace(size_a=size_fn("a", 20), size_b=size_fn("b", 20), size_none=size_fn("none", 0))
    monkeypatch.setattr(ops._lib, "lib", lambda: stub)
    monkeypatch.setattr(ops, "_search_ws", {})
    ws = ops._search_workspace("size_a", "cpu", (1, 2, 3), "a: outside")
    assert ws.dtype == torch.int64 and ws.numel() == 3 and calls == [("a", (1, 2, 3))]      # 20 bytes: three int64 words
    assert ops._search_workspace("size_a", "cpu", (1, 2, 3), "a: outside") is ws and len(calls) == 1   # a hit asks nothing
    other = ops._search_workspace("size_b", "cpu", (1, 2, 3), "b: outside")
    assert other is not ws and other.data_ptr() != ws.data_ptr()
    assert ops._search_workspace("size_a", "cpu", (1, 2, 4), "a: outside") is not ws
    assert sorted(k[0] for k in ops._search_ws) == ["size_a", "size_a", "size_b"]
    with pytest.raises(CapnetError, match="who: n=9 outside the limits"):
        ops._search_workspace("size_none", "cpu", (9,), "who: n=9 outside the limits")
    assert len(ops._search_ws) == 3                    # a refused size caches nothing
