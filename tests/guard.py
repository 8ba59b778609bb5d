"""Guard bands around kernel operands (test infrastructure, a plain module like tests/replay.py).

An `Arena` carves every operand of a call out of ONE larger allocation of its own, so that whatever a kernel reads or writes within a tile of
the operand lands in bytes the test owns and knows:

  [ halo | view: rows x (cols + row gap) | halo ]        halo = max(1 MiB, 256 rows of the view's row stride) on each side

The view starts 16 bytes past a 256-byte boundary (the alignment the C ABI states, not the one the torch allocator happens to give), its
rows may be further apart than they are wide (lda > k, ldc > n, ldq > 3 H).  Halos, row gaps and pad rows of INPUTS hold the NaN of their
type (`POISON`), so a value fetched from there and let into a sum shows in the result; those of OUTPUTS and of the workspace hold seeded
random bytes (a constant could be what a stray store writes), and `Arena.check()` compares every such byte with a saved copy and names the
first one that changed as (buffer, row, column).  `assert_same` does the same for a result against its reference.  Works on any device:
tests/test_guard_cpu.py shows with torch "kernels" on the CPU that each kind of mistake is caught where it happened."""
from __future__ import annotations

from typing import List, Optional

import torch

HALO_MIN_BYTES = 1 << 20
HALO_ROWS = 256                 # the tallest tile of any kernel of the library
ALIGN, ALIGN_MOD = 256, 16      # a view starts at ALIGN_MOD mod ALIGN bytes

# the byte pattern (one element, little endian) that halos, gaps and pad rows of an input of each kind are filled with
POISON = {
    "bf16": bytes([0xC0, 0x7F]),                # 0x7FC0
    "fp16": bytes([0x00, 0x7E]),                # 0x7E00
    "fp32": bytes([0x00, 0x00, 0xC0, 0x7F]),    # quiet NaN: scale vectors too
    "e4m3": bytes([0x7F]),                      # the NaN of OCP e4m3
    "e8m0": bytes([0xFF]),                      # the NaN of an E8M0 scale byte
    "mxfp4": bytes([0x77]),                     # e2m1 has no NaN: two 6.0 nibbles, the scale bytes next to them are poisoned
    "int": bytes([0xFF, 0xFF, 0xFF, 0x7F]),     # int32 / int64 index inputs: INT_MAX halves, an index no table holds
}
_KIND_OF = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32", torch.int32: "int", torch.int64: "int"}


class GuardError(AssertionError):
    """a guard byte changed, or a result differs from its reference: `buffer`, `row`, `col` say where (rows and columns of the view, in
    elements; a row < 0 or >= rows lies in a halo, a column >= cols in a row gap)"""

    def __init__(self, buffer: str, row: int, col: int, what: str):
        super().__init__(f"{what}: buffer '{buffer}', row {row}, column {col}")
        self.buffer, self.row, self.col = buffer, row, col


class View:
    """one operand: `t` is the [rows, cols] tensor (row stride `ld` elements) inside `buf`, `ptr` its address"""

    def __init__(self, name, buf, off, rows, cols, ld, dtype, is_input, kind=None):
        self.name, self.buf, self.off, self.rows, self.cols, self.ld, self.dtype, self.is_input = name, buf, off, rows, cols, ld, dtype, is_input
        self.kind = kind                # an input's POISON key; None for outputs
        self.esz = torch.empty(0, dtype=dtype).element_size()
        self.t = buf[off: off + rows * ld * self.esz].view(dtype).view(rows, ld)[:, :cols]
        self.ptr = buf.data_ptr() + off
        self.guard = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
        self.guard[off: off + rows * ld * self.esz].view(rows, ld * self.esz)[:, : cols * self.esz] = False
        self.saved: Optional[torch.Tensor] = None

    @property
    def nbytes(self) -> int:
        return self.rows * self.ld * self.esz

    def payload_bytes(self) -> torch.Tensor:
        """the view's own extent (rows x ld, gaps included) as a flat uint8 tensor"""
        return self.buf[self.off: self.off + self.nbytes]

    def add_guard(self, byte_offsets: torch.Tensor, poison: Optional[bytes] = None) -> None:
        """makes bytes INSIDE the view (offsets from its start: a pad row of a packed layout) guard bytes; an input's get `poison`"""
        idx = byte_offsets.to(self.buf.device).long() + self.off
        self.guard[idx] = True
        if poison is not None:
            pat = torch.tensor(list(poison), dtype=torch.uint8, device=self.buf.device)
            self.buf[idx] = pat[(idx - self.off) % len(poison)]

    def locate(self, byte_index: int):
        rel = byte_index - self.off
        if self.rows == 1 and rel >= 0:                 # a flat buffer (workspace, vector): the offset from its start
            return 0, int(rel // self.esz)
        row = rel // (self.ld * self.esz)
        return int(row), int((rel - row * self.ld * self.esz) // self.esz)


class Arena:
    def __init__(self, device, seed: int = 0):
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device).manual_seed(0x5EED + seed)
        self.views: List[View] = []

    # ---- allocation
    def _alloc(self, name, rows, cols, ld, dtype, is_input, align_mod, fill: Optional[bytes], halo_bytes: Optional[int] = None, kind=None):
        esz = torch.empty(0, dtype=dtype).element_size()
        ld = cols if ld is None else ld
        assert ld >= cols and rows >= 1 and (cols >= 1 or rows == 1) and align_mod % esz == 0      # (an empty flat view: a workspace of 0 bytes)
        # (a flat buffer -- one row: a vector, a workspace -- has no row stride to speak of: 1 MiB, or what the caller asks for)
        halo = max(HALO_MIN_BYTES, HALO_ROWS * ld * esz if rows > 1 else 0, halo_bytes or 0)
        halo = (halo + 15) // 16 * 16
        total = (halo + ALIGN + rows * ld * esz + halo + 15) // 16 * 16
        if fill is None:
            buf = torch.randint(0, 256, (total,), dtype=torch.uint8, device=self.device, generator=self.gen)
        else:
            buf = torch.tensor(list(fill) * (16 // len(fill)), dtype=torch.uint8, device=self.device).repeat(total // 16)
        off = halo + (align_mod - (buf.data_ptr() + halo)) % ALIGN
        v = View(name, buf, off, rows, cols, ld, dtype, is_input, kind)
        assert v.ptr % ALIGN == align_mod % ALIGN and off >= halo and total - (off + v.nbytes) >= halo
        self.views.append(v)
        return v

    def input(self, name: str, values: torch.Tensor, ld: Optional[int] = None, kind: Optional[str] = None, align_mod: int = ALIGN_MOD) -> View:
        """a [rows, cols] input holding `values`; everything around them is POISON[kind] (kind: by dtype, or "e4m3" / "e8m0" / "mxfp4"
        for uint8 operands)"""
        values = values.reshape(1, -1) if values.dim() == 1 else values
        kind = kind or _KIND_OF[values.dtype]
        v = self._alloc(name, values.shape[0], values.shape[1], ld, values.dtype, True, align_mod, POISON[kind], kind=kind)
        v.t.copy_(values)
        return v

    def output(self, name: str, rows: int, cols: int, dtype, ld: Optional[int] = None, init: Optional[torch.Tensor] = None,
               align_mod: int = ALIGN_MOD) -> View:
        """a [rows, cols] output; halos, gaps AND the not yet written payload are seeded random bytes (`init`: the payload's start values)"""
        v = self._alloc(name, rows, cols, ld, dtype, False, align_mod, None)
        if init is not None:
            v.t.copy_(init.reshape(rows, cols))
        return v

    def workspace(self, name: str, nbytes: int, align_mod: int = ALIGN_MOD, halo_bytes: Optional[int] = None) -> View:
        """`nbytes` of workspace as a one-row uint8 view: the bytes from nbytes on are a guard region (`halo_bytes`: its depth where
        1 MiB is less than one unit of what the callee lays out there, e.g. an m x n fp32 slab)"""
        return self._alloc(name, 1, nbytes, None, torch.uint8, False, align_mod, None, halo_bytes)

    # ---- checking
    def snapshot(self) -> None:
        """call after the operands are set up and before the kernel runs"""
        for v in self.views:
            v.saved = v.buf.clone()

    def check(self) -> None:
        """every guard byte of every view, and every byte of an input, is what snapshot() saw"""
        for v in self.views:
            assert v.saved is not None, "Arena.check() without snapshot()"
            if torch.equal(v.buf, v.saved):
                continue
            diff = v.buf != v.saved
            if not v.is_input:
                diff &= v.guard
            if bool(diff.any()):
                row, col = v.locate(int(diff.nonzero()[0]))
                raise GuardError(v.name, row, col, "an input was modified" if v.is_input else "a byte outside the output's extent was written")


def packed_row_offsets(row: int, row_bytes: int) -> torch.Tensor:
    """byte offsets of one row in the packed operand layout (atspeed_pack_rows): an odd row count's pad row is row `rows`"""
    b = torch.arange(row_bytes)
    return ((row >> 1) * (row_bytes // 64) + (b >> 6)) * 128 + (row & 1) * 64 + (b & 63)


def packed_gap_offsets(rows: int, col_bytes: int, row_bytes: int) -> torch.Tensor:
    """byte offsets of the row gap (bytes col_bytes .. row_bytes - 1 of rows 0 .. rows - 1) of a packed buffer whose rows are row_bytes apart"""
    r = torch.arange(rows)[:, None]
    b = torch.arange(col_bytes, row_bytes)[None, :]
    return (((r >> 1) * (row_bytes // 64) + (b >> 6)) * 128 + (r & 1) * 64 + (b & 63)).reshape(-1)


def assert_same(name: str, got: torch.Tensor, want: torch.Tensor) -> None:
    """bit equality of two [rows, cols] tensors of one dtype (NaNs compare by their bits); names the first element that differs"""
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    g = got.contiguous().view(torch.uint8).reshape(got.shape[0], -1)
    w = want.contiguous().view(torch.uint8).reshape(want.shape[0], -1).to(g.device)
    if torch.equal(g, w):
        return
    row, byte = (int(x) for x in (g != w).nonzero()[0])
    raise GuardError(name, row, byte // got.element_size(), "the result differs from the call on dense operands")
