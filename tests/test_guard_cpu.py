"""tests/guard.py bites: torch "kernels" on CPU tensors behind the Arena interface the GPU tests use (tests/test_guard_bands_gpu.py).  Each of
the three deliberately wrong kernels makes one of the mistakes the guard bands exist for -- a store one row past m, a 16-byte store into
a row gap, a gap column let into a sum -- and must be caught with the buffer, row and column named; the correct kernel passes."""
import pytest
import torch

from tests import guard
from tests.guard import Arena, GuardError

M, N, K, GAP = 37, 24, 40, 8          # 16-bit operands: the row gap is a multiple of 8 elements and no multiple of 64


def _gemm_ok(a: guard.View, w: guard.View, c: guard.View):
    """C = A W^T over the stated extents only, through the views' strides"""
    c.t.copy_((a.t.float() @ w.t.float().T).to(c.dtype))


def _gemm_row_past_m(a, w, c):
    _gemm_ok(a, w, c)
    flat = c.buf[c.off:].view(c.dtype)
    flat[M * c.ld + 3] = 1.0                                     # one element of "row m"


def _gemm_chunk_into_gap(a, w, c):
    _gemm_ok(a, w, c)
    c.buf[c.off + 5 * c.ld * c.esz + N * c.esz:][:16] = 0        # a whole 16-byte store at a column tile that straddles N, row 5


def _gemm_sums_a_gap_column(a, w, c):
    rows = a.buf[a.off: a.off + a.nbytes].view(a.dtype).view(a.rows, a.ld)
    wide = torch.cat((w.t.float(), torch.zeros(w.rows, 1)), 1)   # "garbage x 0": the column past k meets a zero weight
    c.t.copy_((rows[:, : K + 1].float() @ wide.T).to(c.dtype))


def _operands(dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(3)
    a_vals = torch.randn(M, K, generator=g).to(dtype)
    w_vals = torch.randn(N, K, generator=g).to(dtype)
    ar = Arena("cpu")
    a = ar.input("a", a_vals, ld=K + GAP)
    w = ar.input("w", w_vals)
    c = ar.output("c", M, N, dtype, ld=N + GAP)
    ar.snapshot()
    want = (a_vals.float() @ w_vals.float().T).to(dtype)
    return ar, a, w, c, want


def test_arena_layout_alignment_poison_and_sentinel():
    ar, a, w, c, _ = _operands()
    for v in (a, w, c):
        assert v.ptr % 256 == 16
        halo = max(1 << 20, 256 * v.ld * v.esz)
        assert v.off >= halo and v.buf.numel() - (v.off + v.nbytes) >= halo
        assert v.t.stride(0) == v.ld and v.t.data_ptr() == v.ptr
    whole = a.buf.view(torch.bfloat16)
    assert bool(torch.isnan(whole[: a.off // 2]).all()) and bool(torch.isnan(whole[(a.off + a.nbytes) // 2:]).all())      # halos
    rows = a.buf[a.off: a.off + a.nbytes].view(torch.bfloat16).view(M, K + GAP)
    assert bool(torch.isnan(rows[:, K:]).all()) and not bool(torch.isnan(rows[:, :K]).any())                              # row gaps
    assert bytes(a.buf[:2].tolist()) == guard.POISON["bf16"]
    assert (K + GAP) % 8 == 0 and GAP % 64 != 0
    # an output's surroundings are random bytes, different ones per buffer and the same ones per seed
    assert len(set(c.buf[:4096].tolist())) > 100
    ar2 = Arena("cpu")
    ar2.input("a", a.t.clone(), ld=K + GAP); ar2.input("w", w.t.clone())
    c2 = ar2.output("c", M, N, torch.bfloat16, ld=N + GAP)
    assert torch.equal(c2.buf, c.buf)
    for kind, pat in guard.POISON.items():
        dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32, "int": torch.int32}.get(kind, torch.uint8)
        v = Arena("cpu").input("x", torch.zeros(3, 16, dtype=dt), ld=24, kind=kind)
        assert bytes(v.buf[v.off - len(pat): v.off].tolist()) == pat and bytes(v.buf[v.off + 16 * v.esz:][: len(pat)].tolist()) == pat
        if kind in ("bf16", "fp16", "fp32"):
            assert bool(torch.isnan(v.buf[: v.off].view(dt)).all())
    assert bool(torch.isnan(torch.tensor([0x7F], dtype=torch.uint8).view(torch.float8_e4m3fn).float()).all())


def test_correct_kernel_passes():
    ar, a, w, c, want = _operands()
    _gemm_ok(a, w, c)
    ar.check()
    guard.assert_same("c", c.t, want)


def test_store_one_row_past_m_is_caught_where_it_happened():
    ar, a, w, c, want = _operands()
    _gemm_row_past_m(a, w, c)
    guard.assert_same("c", c.t, want)                            # the result itself is right: only the guard band sees it
    with pytest.raises(GuardError) as e:
        ar.check()
    assert (e.value.buffer, e.value.row, e.value.col) == ("c", M, 3)


def test_sixteen_byte_store_into_a_row_gap_is_caught_where_it_happened():
    ar, a, w, c, want = _operands()
    _gemm_chunk_into_gap(a, w, c)
    guard.assert_same("c", c.t, want)
    with pytest.raises(GuardError) as e:
        ar.check()
    assert (e.value.buffer, e.value.row, e.value.col) == ("c", 5, N)


def test_gap_column_in_a_sum_is_caught_where_it_happened():
    ar, a, w, c, want = _operands()
    _gemm_sums_a_gap_column(a, w, c)
    ar.check()                                                   # nothing stray was written ...
    with pytest.raises(GuardError) as e:
        guard.assert_same("c", c.t, want)                        # ... but NaN x 0 reached every sum
    assert (e.value.buffer, e.value.row, e.value.col) == ("c", 0, 0)
    assert bool(torch.isnan(c.t.float()).all())


def test_modified_input_pad_row_and_workspace_overrun_are_caught():
    ar = Arena("cpu")
    x = ar.input("xp", torch.ones(4, 64, dtype=torch.uint8), kind="e4m3")          # 3 rows of 64 bytes packed: row 3 is the pad row
    x.add_guard(guard.packed_row_offsets(3, 64), guard.POISON["e4m3"])
    assert x.payload_bytes().view(2, 2, 64)[1, 1].tolist() == [0x7F] * 64 and int(x.payload_bytes().view(2, 2, 64)[1, 0].sum()) == 64
    ws = ar.workspace("ws", 1000)
    out = ar.output("cp", 4, 64, torch.uint8)
    out.add_guard(guard.packed_row_offsets(3, 64))
    ar.snapshot()
    ws.payload_bytes()[:1000] = 1
    out.payload_bytes().view(2, 2, 64)[:, 0] = 7; out.payload_bytes().view(2, 2, 64)[0, 1] = 7
    ar.check()
    ws.buf[ws.off + 1000] ^= 0xFF                                                  # one byte past workspace_bytes
    with pytest.raises(GuardError) as e:
        ar.check()
    assert (e.value.buffer, e.value.row, e.value.col) == ("ws", 0, 1000)
    ws.buf[ws.off + 1000] ^= 0xFF
    empty = Arena("cpu")
    w0 = empty.workspace("ws0", 0)                                                   # workspace_bytes = 0: byte 0 is a guard byte already
    empty.snapshot()
    w0.buf[w0.off] ^= 0xFF
    with pytest.raises(GuardError) as e:
        empty.check()
    assert (e.value.buffer, e.value.row, e.value.col) == ("ws0", 0, 0) and w0.kind is None and x.kind == "e4m3"
    gap = guard.packed_gap_offsets(3, 64, 128)                                     # 3 rows of 64 payload bytes, 128 apart
    assert gap.numel() == 3 * 64 and gap[:2].tolist() == [128, 129] and int(gap[64]) == 128 + 64 and int(gap[128]) == 256 + 128
    out.payload_bytes().view(2, 2, 64)[1, 1, 9] ^= 0xFF                             # the output's pad row
    with pytest.raises(GuardError) as e:
        ar.check()
    assert e.value.buffer == "cp" and e.value.row * 64 + e.value.col == 3 * 64 + 9
    out.payload_bytes().view(2, 2, 64)[1, 1, 9] ^= 0xFF
    x.t[0, 0] = 2                                                                   # an input is read-only
    with pytest.raises(GuardError) as e:
        ar.check()
    assert (e.value.buffer, e.value.row, e.value.col) == ("xp", 0, 0)
