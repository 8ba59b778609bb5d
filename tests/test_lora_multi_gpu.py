"""Several resident LoRA adapters in one batch (atspeed_llama_add_lora) on the GPU.  The segmented kernels are pinned to the
single-adapter entry points -- which tests/test_lora_gpu.py pins to fp64 -- bit for bit, per segment, over layouts whose 16-row tiles mix
adapters; once directly to the fp64 rule.  Then whole forwards, lock-step batches, sessions and target_generate batches whose users name
different adapters against the single calls and the oracle, the 16-bit and W8A8 engines at the Llama-7B width bit for bit against the
model-wide adapter, captured graphs, and the lifecycle.  Run with -m gpu on the MI355X box."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import atspeed_amd
from atspeed_amd import _lib, lora as L, synth
from atspeed_amd.beamSD import BSSD, BSSD_batch, release_decoders, target_generate, target_generate_batch
from atspeed_amd.model import HipLlama, vis_bits_from_bool
from oracle import beamsd_ref as R
from oracle.llama_ref import RefLlama
from tests import guard, lora_ref as LR, segs_cases as SC
from tests.golden.cases import CASES, build_case_inputs
from tests.guard import assert_same

TD = SC.TORCH
SCORE_TOL = 1e-3                                   # the fp32 bar (tests/test_bssd_gpu.py, tests/test_lora_gpu.py)
U_LD = 3 * _lib.LORA_MAX_RANK                      # the segmented kernels' fixed row stride of u


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _st():
    return _lib.stream_ptr()


def _fmt(x, dtype):
    t = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(TD[dtype])
    return t.double().numpy(), t


# ------------------------------------------------------------------ 1. the two segmented kernels against the single-adapter entry points
# slot 1: rank 8 on q, v; slot 2: rank 40 on q, k, v, scaling 0.5; slot 3: rank 64 on v only
SLOTS = {1: dict(rank=8, modules="qv", scaling=2.0), 2: dict(rank=40, modules="qkv", scaling=0.5), 3: dict(rank=64, modules="v", scaling=1.0)}
# A: 64 rows; the first 16-row tile holds three different adapters, none among them, and a segment straddles tiles.  B: 35 rows, a partial
# last tile, and the same adapter on both sides of another one inside a tile
LAYOUTS = {"A": ([5, 4, 7, 19, 16, 1, 12], [1, 2, 0, 2, 1, 3, 3]), "B": ([3, 30, 2], [2, 1, 2])}
# both slots pad to R16 = 32: rank 24 on q, v and rank 32 on k only.  25 rows: the first 16-row tile mixes both adapters, the same adapter sits
# on both sides of the other one, the last tile is partial
SLOTS_R32 = {1: dict(rank=24, modules="qv", scaling=2.0), 2: dict(rank=32, modules="k", scaling=0.5)}
LAYOUTS["R32"] = ([7, 9, 9], [1, 2, 1])
SHAPES_R32 = [(4, 64, "bf16"), (4, 64, "fp16"), (5, 40, "bf16")]
SHAPES = [(4, 64, "bf16"), (4, 64, "fp16"), (12, 64, "bf16"), (12, 64, "fp16"), (5, 40, "bf16"), (5, 40, "fp16"), (12, 64, "fp32")]
LAYER = 1


class Segs:
    """the segments of a layout: own positions (tree tokens: repeats; one beyond the table) and slots (a permutation: row != slot)"""

    def __init__(self, n_tok, H, td):
        rng = np.random.default_rng(1234 + len(n_tok))
        self.n_tok, self.n, self.H, self.td = list(n_tok), len(n_tok), H, td
        self.row0 = np.concatenate([[0], np.cumsum(n_tok)])
        self.total = int(self.row0[-1])
        self.pos = [np.arange(3 * i, 3 * i + t) for i, t in enumerate(n_tok)]
        self.pos[1][-2:] = self.pos[1][0]
        self.pos[-1][0] = SC.MAX_POS + 7
        self.slots = [rng.permutation(SC.MAX_SLOTS)[:t] for t in n_tok]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()
        self.d_pos, self.d_slots = [dev(p) for p in self.pos], [dev(s) for s in self.slots]

    def caches(self, n=None):
        fill = torch.full((SC.LAYERS, SC.MAX_SLOTS, self.H), 3.0, dtype=self.td, device="cuda")
        return [fill.clone() for _ in range(n or self.n)], [fill.clone() for _ in range(n or self.n)]

    def args(self, kc, vc, only=None):
        """ATSPEED_SEGMENTS of all segments, or of segment `only` alone (kc / vc then hold its caches only)"""
        ix = list(range(self.n)) if only is None else [only]
        n = len(ix)
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        cnt = lambda v: (C.c_int32 * n)(*v)
        self._keep = [None, arr([self.d_pos[i] for i in ix]), arr([self.d_slots[i] for i in ix]), None, arr(kc), arr(vc),
                      cnt([self.n_tok[i] for i in ix]), cnt([SC.MAX_SLOTS] * n), cnt([0] * n)]
        return [n] + self._keep

    def rows(self, i):
        return slice(int(self.row0[i]), int(self.row0[i + 1]))

    def row_adapter(self, adapters):
        return np.concatenate([[a] * t for a, t in zip(adapters, self.n_tok)])


def _slot_weights(rng, H, dtype, slots):
    """per slot: (r16, a_cat64, a_cat tensor, {module: (b64, b tensor)}) laid out as the library lays its copies out (pad rows / columns zero)"""
    out = {}
    for s, sp in slots.items():
        rank, r16 = sp["rank"], (sp["rank"] + 15) // 16 * 16
        a = np.zeros((3 * r16, H), dtype=np.float32)
        bs = {}
        for k, m in enumerate("qkv"):
            if m in sp["modules"]:
                a[k * r16: k * r16 + rank] = rng.standard_normal((rank, H)) / np.sqrt(H)
                b = np.zeros((H, r16), dtype=np.float32)
                b[:, :rank] = rng.standard_normal((H, rank)) * 0.3
                bs[m] = _fmt(b, dtype)
        out[s] = (r16, *_fmt(a, dtype), bs)
    return out


class KernelCase:
    """inputs of one (layout, shape, dtype) on the device, the slot table, and the two segmented kernels' results"""

    def __init__(self, lib, layout, n_heads, head_dim, dtype, slots=SLOTS):
        self.slots = slots
        self.lib, self.dtype, self.td, self.code = lib, dtype, TD[dtype], _lib.dtype_code(TD[dtype])
        self.n_heads, self.head_dim, self.H = n_heads, head_dim, n_heads * head_dim
        n_tok, self.adapters = LAYOUTS[layout]
        H = self.H
        self.S = S = Segs(n_tok, H, self.td)
        rng = np.random.default_rng(97 * H + len(n_tok) + len(dtype))
        self.h64, self.h_t = _fmt(rng.standard_normal((S.total, H)) * (0.5 + rng.random((S.total, 1)) * 3), dtype)
        self.w64, self.w_t = _fmt(1 + 0.1 * rng.standard_normal(H), dtype)
        self.qkv64, self.qkv_t = _fmt(rng.standard_normal((S.total, 3 * H)), dtype)
        self.W = _slot_weights(rng, H, dtype, slots)
        self.dev = {s: (w[2].cuda(), {m: b[1].cuda() for m, b in w[3].items()}) for s, w in self.W.items()}
        self.tab = (_lib.LoraSlot * 4)()
        for s, (a, bs) in self.dev.items():
            ptr = lambda m: bs[m].data_ptr() if m in bs else None
            self.tab[s] = _lib.LoraSlot(a.data_ptr(), ptr("q"), ptr("k"), ptr("v"), self.W[s][0], slots[s]["scaling"])
        self.seg_ad = (C.c_int32 * S.n)(*self.adapters)
        cos, sin = (torch.from_numpy(t).cuda() for t in SC.rope_tables(head_dim))
        self.cos, self.sin = cos, sin
        self.loff = LAYER * SC.MAX_SLOTS * H * self.qkv_t.element_size()
        self.tail = (cos.data_ptr(), sin.data_ptr(), self.loff, n_heads, head_dim, SC.MAX_POS, self.code)
        self.hd, self.wd = self.h_t.cuda(), self.w_t.cuda()
        self.poison = torch.tensor(list(guard.POISON[dtype]), dtype=torch.uint8, device="cuda")

    def poisoned_u(self, ar, name):
        vu = ar.output(name, self.S.total, U_LD, self.td)
        vu.payload_bytes().copy_(self.poison.repeat(vu.nbytes // self.poison.numel()))
        return vu

    def shrink_multi(self):
        """-> the u view (guard arena checked: nothing outside [total][192] written, inputs untouched)"""
        ar = guard.Arena("cuda", seed=self.H)
        vh, vw = ar.input("h", self.hd), ar.input("norm_w", self.wd)
        vu = self.poisoned_u(ar, "u")
        ar.snapshot()
        noseg = [None] * 6
        S = self.S
        cnt = lambda v: (C.c_int32 * S.n)(*v)
        _lib.check(self.lib.atspeed_segs_lora_shrink_multi(vh.ptr, vw.ptr, self.tab, 4, vu.ptr, self.H, 1e-6, self.code, self.seg_ad,
                                                           S.n, *noseg, cnt(S.n_tok), cnt([SC.MAX_SLOTS] * S.n), cnt([0] * S.n), _st()))
        torch.cuda.synchronize()
        ar.check()
        return vu

    def shrink_single(self, i):
        """segment i alone through atspeed_lora_shrink with its adapter: [n_tok][3 r16]"""
        a, rows = self.adapters[i], self.S.rows(i)
        r16 = self.W[a][0]
        h = self.hd[rows].contiguous()
        u = torch.empty(self.S.n_tok[i], 3 * r16, dtype=self.td, device="cuda")
        _lib.check(self.lib.atspeed_lora_shrink(h.data_ptr(), self.wd.data_ptr(), self.dev[a][0].data_ptr(), u.data_ptr(), self.S.n_tok[i], self.H,
                                                3 * r16, 1e-6, self.code, _st()))
        torch.cuda.synchronize()
        return u

    def is_poison(self, t):
        """[rows][cols] -> bool [rows][cols]: the element still holds the guard poison"""
        b = t.contiguous().view(torch.uint8).reshape(t.shape[0], t.shape[1], -1)
        return (b == self.poison.to(b.device)).all(-1)


@pytest.fixture(scope="module")
def kernel_cases(lib):
    cache = {}

    def get(layout, n_heads, head_dim, dtype, slots=SLOTS):
        key = (layout, n_heads, head_dim, dtype)
        if key not in cache:
            cache[key] = KernelCase(lib, layout, n_heads, head_dim, dtype, slots)
        return cache[key]
    return get


@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("n_heads,head_dim,dtype", SHAPES, ids=[f"{h * d}_{t}" for h, d, t in SHAPES])
def test_segmented_kernels_equal_the_single_adapter_kernels_per_segment(lib, kernel_cases, layout, n_heads, head_dim, dtype):
    """hidden 256 / 768 (MFMA shrink, vector expand), 200 = 5 x 40 (the scalar 16-bit forms) and fp32: for every segment with adapter a > 0 the
    rows of u, of q and of the K / V caches are bit-identical to atspeed_lora_shrink / atspeed_segs_lora_rope_kv of that segment ALONE with
    adapter a; for adapter 0, q and the caches are bit-identical to atspeed_segs_rope_kv and the segment's u rows still hold the guard
    poison; of an adapted row only [0, 3 r16) of u is written.  The expand is fed the single-adapter kernels' u scattered into a poisoned
    buffer, so that a row of adapter 0 that is read shows as a NaN."""
    _segmented_equal_single(lib, kernel_cases(layout, n_heads, head_dim, dtype))


@pytest.mark.parametrize("n_heads,head_dim,dtype", SHAPES_R32, ids=[f"{h * d}_{t}" for h, d, t in SHAPES_R32])
def test_segmented_kernels_equal_the_single_adapter_kernels_at_a_padded_rank_of_32(lib, kernel_cases, n_heads, head_dim, dtype):
    """the same assertions with SLOTS_R32 on layout R32: lora_shrink_mfma_kernel<6> and the segmented MFMA shrink's 6-tile pass (hidden 256,
    with the vector expand) and the scalar 16-bit forms (200 = 5 x 40); SLOTS pads to 16, 48 and 64 only"""
    _segmented_equal_single(lib, kernel_cases("R32", n_heads, head_dim, dtype, SLOTS_R32))


def _segmented_equal_single(lib, kc_):
    S, H, td = kc_.S, kc_.H, kc_.td
    vu = kc_.shrink_multi()
    u_multi = vu.t.clone()
    u_in = kc_.poisoned_u(guard.Arena("cuda", seed=1), "u_in")
    singles = {}
    for i, a in enumerate(kc_.adapters):
        rows = S.rows(i)
        if a == 0:
            assert bool(kc_.is_poison(u_multi[rows]).all()), f"segment {i} names no adapter: its u rows must not be written"
            continue
        r16 = kc_.W[a][0]
        singles[i] = us = kc_.shrink_single(i)
        assert_same(f"u of segment {i} (adapter {a}) vs atspeed_lora_shrink of the segment alone", u_multi[rows, : 3 * r16], us)
        assert 3 * r16 == U_LD or bool(kc_.is_poison(u_multi[rows, 3 * r16:]).all()), f"segment {i}: columns from 3 r16 on were written"
        assert float(us.float().abs().max()) > 0
        u_in.t[rows, : 3 * r16] = us
    q = kc_.qkv_t.clone().cuda()
    kc, vc = S.caches()
    _lib.check(lib.atspeed_segs_lora_rope_kv_multi(q.data_ptr(), u_in.ptr, kc_.tab, 4, *kc_.tail, kc_.seg_ad, *S.args(kc, vc), _st()))
    torch.cuda.synchronize()
    assert_same("k and v columns of qkv stay the projection's", q[:, H:].cpu(), kc_.qkv_t[:, H:])
    for i, a in enumerate(kc_.adapters):
        rows = S.rows(i)
        q1 = kc_.qkv_t[rows].clone().cuda()
        k1, v1 = S.caches(1)
        if a == 0:
            _lib.check(lib.atspeed_segs_rope_kv(q1.data_ptr(), None, 0, *kc_.tail, *S.args(k1, v1, only=i), _st()))
        else:
            bs = kc_.dev[a][1]
            ptr = [bs[m].data_ptr() if m in bs else None for m in "qkv"]
            _lib.check(lib.atspeed_segs_lora_rope_kv(q1.data_ptr(), singles[i].data_ptr(), *ptr, kc_.W[a][0], kc_.slots[a]["scaling"], *kc_.tail,
                                                     *S.args(k1, v1, only=i), _st()))
        torch.cuda.synchronize()
        assert_same(f"q of segment {i} (adapter {a})", q[rows, :H].cpu(), q1[:, :H].cpu())
        assert_same(f"K cache of segment {i} (adapter {a})", kc[i].view(-1, H).cpu(), k1[0].view(-1, H).cpu())
        assert_same(f"V cache of segment {i} (adapter {a})", vc[i].view(-1, H).cpu(), v1[0].view(-1, H).cpu())
        if a:
            plain = kc_.qkv_t[rows].clone().cuda()
            kp, vp = S.caches(1)
            _lib.check(lib.atspeed_segs_rope_kv(plain.data_ptr(), None, 0, *kc_.tail, *S.args(kp, vp, only=i), _st()))
            torch.cuda.synchronize()
            for m, got, base in (("k", kc[i], kp[0]), ("v", vc[i], vp[0])):
                assert m not in kc_.slots[a]["modules"] or not torch.equal(got, base), f"segment {i}: the adapter must move {m}"


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_segmented_kernels_against_the_fp64_rule(lib, kernel_cases, dtype):
    """layout A at hidden 768 directly against tests/lora_ref.py, per row with the row's adapter and under shrink_ref64's / expand_ref64's own
    bounds (the expand continued from the u the kernel was given, the rotation carried as in tests/test_lora_gpu.py); near ties stay under
    rounding.CAP"""
    kc_ = kernel_cases("A", 12, 64, dtype)
    S, H = kc_.S, kc_.H
    u = kc_.shrink_multi().t.clone()
    row_ad = S.row_adapter(kc_.adapters)
    ties = rows_checked = 0
    for a in SLOTS:
        rows = np.flatnonzero(row_ad == a)
        r16, a64 = kc_.W[a][0], kc_.W[a][1]
        ref, bound, n_tie = LR.shrink_ref64(kc_.h64[rows], kc_.w64, a64, 1e-6, dtype)
        err = np.abs(u[rows, : 3 * r16].double().cpu().numpy() - ref)
        print(f"segmented shrink {dtype} slot {a}: worst |err| / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all(), (a, np.argwhere(err > bound)[:3].tolist())
        ties += n_tie
        rows_checked += len(rows)
    assert ties / (rows_checked * H) <= LR.R.CAP
    q = kc_.qkv_t.clone().cuda()
    kc, vc = S.caches()
    _lib.check(lib.atspeed_segs_lora_rope_kv_multi(q.data_ptr(), u.data_ptr(), kc_.tab, 4, *kc_.tail, kc_.seg_ad, *S.args(kc, vc), _st()))
    torch.cuda.synchronize()
    pos = np.concatenate(S.pos)
    gather = lambda caches: np.concatenate([caches[i][LAYER].double().cpu().numpy()[S.slots[i]] for i in range(S.n)])
    got = {"q": q[:, :H].double().cpu().numpy(), "k": gather(kc), "v": gather(vc)}
    u64 = u.double().cpu().numpy()
    for a, sp in SLOTS.items():
        rows = np.flatnonzero(row_ad == a)
        r16 = kc_.W[a][0]
        for k, m in enumerate("qkv"):
            if m not in sp["modules"]:
                continue
            base = kc_.qkv64[rows, k * H: (k + 1) * H]
            y, e_y = LR.expand_ref64(base, u64[rows, k * r16: (k + 1) * r16], kc_.W[a][3][m][0], sp["scaling"], dtype)
            if dtype == "fp32":
                e_y = e_y + 2.0 ** -23 * (np.abs(base) + np.abs(y - base))
            assert float(np.abs(y - base).mean()) > 0.05, "the adapter's term must be visible against the base"
            if m == "v":
                ref, bound = y, e_y
            else:
                ref, mag = SC.rope_rotate64(y, pos[rows], kc_.n_heads, kc_.head_dim)
                _, carried = SC.rope_rotate64(e_y, pos[rows], kc_.n_heads, kc_.head_dim)
                bound = LR.rounded_within(ref, carried + SC.ROPE_REL * mag, dtype)
            err = np.abs(got[m][rows] - ref)
            print(f"segmented expand {dtype} slot {a} module {m}: worst |err| / bound {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), (a, m, np.argwhere(err > bound)[:3].tolist())


def test_bare_entry_points_refuse_a_slot_the_table_does_not_hold(lib, kernel_cases):
    kc_ = kernel_cases("B", 4, 64, "bf16")
    S = kc_.S
    u = torch.zeros(S.total, U_LD, dtype=kc_.td, device="cuda")
    bad = (C.c_int32 * S.n)(2, 4, 2)
    cnt = lambda v: (C.c_int32 * S.n)(*v)
    rc = lib.atspeed_segs_lora_shrink_multi(kc_.hd.data_ptr(), kc_.wd.data_ptr(), kc_.tab, 4, u.data_ptr(), kc_.H, 1e-6, kc_.code, bad, S.n,
                                            *([None] * 6), cnt(S.n_tok), cnt([SC.MAX_SLOTS] * S.n), cnt([0] * S.n), _st())
    assert rc == _lib.ERR_INVALID and b"slot 4" in lib.atspeed_last_error()


# ------------------------------------------------------------------ 2. fp32 engine: the golden case with users on different adapters
def _adapter(dims, seed, r=8, alpha=16, modules=("q", "v"), std=0.1):
    return L.from_tensors(synth.synthetic_lora(dims, seed, r=r, modules=modules, std=std), dims.n_layers, dims.hidden, r, alpha)


KW = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
ASSIGN = ["a", None, "b", "a", "b"]                 # users 0 and 2 share one prompt; user 4 is the one a 2-lane session queues


@pytest.fixture(scope="module")
def world():
    """the golden case's models -- one target with both adapters resident, and for the single calls one per model-wide adapter and a plain
    one -- five users, and each user's own single BSSD call on the model that holds only its adapter"""
    case = [c for c in CASES if c["name"] == "k20_dk40_sigma01"][0]
    ci = build_case_inputs(case)
    td, dd = ci["target_dims"], ci["draft_dims"]
    ads = {"a": _adapter(td, 77), "b": _adapter(td, 78)}
    mk = lambda: HipLlama.from_state_dict(td, ci["target_sd"], torch.float32, num_beams=case["K"], **KW)
    multi = mk().add_lora(ads["a"], "a").add_lora(ads["b"], "b")
    drf = HipLlama.from_state_dict(dd, ci["draft_sd"], torch.float32, num_beams=case["DK"], **KW)
    only = {"a": mk().load_lora(ads["a"]), "b": mk().load_lora(ads["b"]), None: mk()}
    prompts = [ci["prompt"], synth.synthetic_prompt(23, 901), ci["prompt"], synth.synthetic_prompt(28, 902), synth.synthetic_prompt(33, 903)]
    inputs = [{"input_ids": torch.from_numpy(p)[None].cuda()} for p in prompts]
    a = (case["gamma"], case["max_new_tokens"])
    single = [BSSD(only[name], drf, inp, *a, prefix_allowed_tokens_fn=ci["fn"]) for name, inp in zip(ASSIGN, inputs)]
    for m in only.values():
        release_decoders(m)
    return dict(case=case, ci=ci, ads=ads, multi=multi, drf=drf, prompts=prompts, inputs=inputs, a=a, single=single, only=only)


def _same_as_single(what, single, outs, atol=1e-4):
    for u, (s, o) in enumerate(zip(single, outs)):
        assert torch.equal(s["beam_sequence"], o["beam_sequence"]), (what, u)
        np.testing.assert_allclose(s["beam_scores"].cpu().numpy(), o["beam_scores"].cpu().numpy(), atol=atol, rtol=0)
        assert (s["n_run"], s["total_accept_steps"], s["accept_steps"]) == (o["n_run"], o["total_accept_steps"], o["accept_steps"]), (what, u)


def test_fp32_forward_batch_with_an_adapter_per_sequence(world):
    """three sequences in one forward under [a, None, b]: each one's logits <= 1e-3 of the reference with that adapter (or none), which the
    adapters move by far more; 2 adapter launches per layer, no fused RoPE"""
    ci, m = world["ci"], world["multi"]
    dims, V = ci["target_dims"], ci["target_dims"].vocab_size
    g = torch.Generator().manual_seed(5)
    names, seqs, raw = ["a", None, "b"], [], []
    for i in range(3):
        P, B = 21 + 9 * i, 14
        T = P + B
        ids = torch.randint(3, V, (T,), generator=g).to(torch.int32)
        vis = torch.zeros(T, T, dtype=torch.bool)
        vis[:P, :P] = torch.tril(torch.ones(P, P, dtype=torch.bool))
        vis[P:, :P] = True
        vis[P:, P:] = torch.eye(B, dtype=torch.bool)
        vis[P:, 2 + i] = False
        pos = torch.cat((torch.arange(P), torch.full((B,), P))).to(torch.int32)
        raw.append((ids, pos, torch.arange(T, dtype=torch.int32), vis))
        seqs.append((ids, pos, raw[-1][2], vis_bits_from_bool(vis, 512), T, B + 1))
    m.lora_launches(reset=True), m.rope_fused_launches(reset=True)
    outs = [o.cpu() for o in m.forward_raw_batch(seqs, adapters=names)]
    assert m.lora_launches() == 2 * dims.n_layers and m.rope_fused_launches() == 0
    for i, name in enumerate(names):
        plain = RefLlama(dims, ci["target_sd"], max_slots=512).forward(*raw[i], n_logit_rows=raw[i][0].numel() - (21 + 9 * i) + 1)
        if name is None:
            want = plain
        else:
            want = LR.LoraRefLlama(dims, ci["target_sd"], max_slots=512).set_lora(world["ads"][name]).forward(*raw[i], n_logit_rows=plain.shape[0])
            assert float((want - plain).abs().max()) > 100 * SCORE_TOL
        err = float((outs[i] - want).abs().max())
        print(f"forward_batch sequence {i} under adapter {name}: max err {err:.2e}")
        assert err <= SCORE_TOL
    with pytest.raises(ValueError):
        m.forward_raw_batch(seqs, adapters=["a"])
    with pytest.raises(KeyError):
        m.forward_raw_batch(seqs, adapters=["a", "zzz", None])


def test_fp32_bssd_batch_with_an_adapter_per_user(world):
    """BSSD_batch of 4 users under [a, None, b, a], users 0 and 2 on the SAME prompt: every user's tokens, n_run and accept_steps equal its own
    single BSSD call on a model holding only that adapter model-wide (or none), scores within 1e-4; tokens equal the oracle's BSSD on the LoRA
    reference, scores within 1e-3; users 0 and 2 return different items -- a build that ignores the per-user slot fails there."""
    w = world
    ci, case = w["ci"], w["case"]
    w["multi"].lora_launches(reset=True)
    bat = BSSD_batch(w["multi"], w["drf"], w["inputs"][:4], *w["a"], prefix_allowed_tokens_fn=ci["fn"], adapters=ASSIGN[:4])
    assert w["multi"].lora_launches() > 0
    _same_as_single("batch", w["single"][:4], bat)
    P0 = len(w["prompts"][0])
    assert bat[0]["beam_sequence"][:, P0:].tolist() != bat[2]["beam_sequence"][:, P0:].tolist(), "users 0 and 2 differ in their adapter alone"
    for u in range(4):
        tgt = LR.LoraRefLlama(ci["target_dims"], ci["target_sd"])
        if ASSIGN[u] is not None:
            tgt.set_lora(w["ads"][ASSIGN[u]])
        ref = R.BSSD(tgt, RefLlama(ci["draft_dims"], ci["draft_sd"]), w["prompts"][u], case["gamma"], case["max_new_tokens"], case["K"], case["DK"], ci["fn"])
        P = len(w["prompts"][u])
        assert bat[u]["beam_sequence"][:, P:].cpu().tolist() == ref["beam_sequence"][:, P:].tolist(), u
        np.testing.assert_allclose(bat[u]["beam_scores"].cpu().numpy(), ref["beam_scores"].numpy(), atol=SCORE_TOL, rtol=0)
    # a later call that names nobody runs every user without an adapter: the decoders do not keep the assignment
    none = BSSD_batch(w["multi"], w["drf"], w["inputs"][:2], *w["a"], prefix_allowed_tokens_fn=ci["fn"])
    assert torch.equal(none[1]["beam_sequence"], w["single"][1]["beam_sequence"])
    assert not torch.equal(none[0]["beam_sequence"], w["single"][0]["beam_sequence"])
    one = BSSD(w["multi"], w["drf"], w["inputs"][2], *w["a"], prefix_allowed_tokens_fn=ci["fn"], adapter="b")
    _same_as_single("one user", [w["single"][2]], [one])
    release_decoders(w["multi"], w["drf"])


def test_fp32_session_lanes_carry_the_adapter_with_the_user(world):
    """the five users through lanes=2 (three queue, whichever lane frees first takes the next): the single calls' results, and the session
    allocates nothing after its creation"""
    w = world
    ses = BSSD_batch(w["multi"], w["drf"], w["inputs"], *w["a"], prefix_allowed_tokens_fn=w["ci"]["fn"], lanes=2, adapters=ASSIGN)
    _same_as_single("lanes=2", w["single"], ses)
    c = ses[0]["session_counters"]
    assert c["allocs_after_create"] == 0 and c["users_retired"] == 5, c
    release_decoders(w["multi"], w["drf"])


def test_fp32_target_generate_batch_with_an_adapter_per_user(world):
    w = world
    fn, L_ = w["ci"]["fn"], w["case"]["max_new_tokens"]
    bat = target_generate_batch(w["multi"], w["inputs"][:4], L_, prefix_allowed_tokens_fn=fn, adapters=ASSIGN[:4])
    for u in range(4):
        one = target_generate(w["multi"], w["inputs"][u], L_, prefix_allowed_tokens_fn=fn, adapter=ASSIGN[u])
        mw = target_generate(w["only"][ASSIGN[u]], w["inputs"][u], L_, prefix_allowed_tokens_fn=fn)
        assert torch.equal(bat[u]["beam_sequence"], one["beam_sequence"]) and torch.equal(one["beam_sequence"], mw["beam_sequence"]), u
        np.testing.assert_allclose(bat[u]["beam_scores"].cpu().numpy(), one["beam_scores"].cpu().numpy(), atol=1e-4, rtol=0)
        np.testing.assert_allclose(one["beam_scores"].cpu().numpy(), mw["beam_scores"].cpu().numpy(), atol=1e-4, rtol=0)
    assert not torch.equal(bat[0]["beam_sequence"], bat[2]["beam_sequence"])
    release_decoders(w["multi"], *w["only"].values())


def test_captured_graph_follows_the_users_adapters(world):
    """graphs on: two users on ONE prompt under [a, b], often enough for the shapes to be captured and replayed, then under [b, a]: the
    results swap with the adapters (the slot is data in the segment table, not part of the captured launches)"""
    w = world
    fn = w["ci"]["fn"]
    inputs = [w["inputs"][0], w["inputs"][0]]
    with _lib.switches(graphs=1):
        ab = [BSSD_batch(w["multi"], w["drf"], inputs, *w["a"], prefix_allowed_tokens_fn=fn, adapters=["a", "b"]) for _ in range(3)]
        ba = BSSD_batch(w["multi"], w["drf"], inputs, *w["a"], prefix_allowed_tokens_fn=fn, adapters=["b", "a"])
        torch.cuda.synchronize()
    want = [w["single"][0], w["single"][2]]                               # the shared prompt under a, under b
    for outs in ab:
        _same_as_single("graphs [a, b]", want, outs)
    _same_as_single("graphs [b, a]", want[::-1], ba)
    assert not torch.equal(ba[0]["beam_sequence"], ba[1]["beam_sequence"])
    release_decoders(w["multi"], w["drf"])


# ------------------------------------------------------------------ 3. bf16 and W8A8 at the Llama-7B width: bit for bit the model-wide adapter
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "w8a8"])
def test_16bit_target_generate_batch_is_bit_identical_to_the_model_wide_adapter(fp8):
    """hidden 4096 / 32 x 128 / 2 layers: target_generate_batch of 3 users under [a, b, None] -- every user advances one position per forward,
    so the token counts and with them the GEMM kernels do not depend on the assignment.  User 0's sequences and scores are bit-identical to
    the same batch with a loaded model-wide, user 1's to the same batch with b model-wide, user 2's to the all-None assignment on the model
    that still holds the slots (the same launch sequence)."""
    V = synth.BEAUTY.vocab_size
    dims = synth.LlamaDims(V, 4096, 2, 32, 11008)
    m = HipLlama.from_synthetic(dims, 2025, std=0.02, head_std=0.05, dtype=torch.bfloat16, num_beams=20, **KW)
    if fp8:
        m.enable_fp8()
    ads = {"a": _adapter(dims, 77, std=0.03), "b": _adapter(dims, 78, r=40, modules=("q", "k", "v"), std=0.03)}
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    inputs = [{"input_ids": torch.from_numpy(synth.synthetic_prompt(40 + 13 * u, 300 + u))[None].cuda()} for u in range(3)]
    run = lambda **kw: target_generate_batch(m, inputs, 4, prefix_allowed_tokens_fn=fn, **kw)
    keep = lambda outs: [(o["beam_sequence"].clone(), o["beam_scores"].clone()) for o in outs]
    m.add_lora(ads["a"], "a").add_lora(ads["b"], "b")
    m.lora_launches(reset=True)
    mixed = keep(run(adapters=["a", "b", None]))
    assert m.lora_launches() == 2 * dims.n_layers * 4
    none = keep(run())
    m.remove_lora("a").remove_lora("b")
    wide = {}
    for name in ("a", "b"):
        m.load_lora(ads[name])
        wide[name] = keep(run())
    m.unload_lora()
    for u, want in enumerate((wide["a"][0], wide["b"][1], none[2])):
        assert torch.equal(mixed[u][0], want[0]), u
        assert_same(f"user {u}'s scores", mixed[u][1][None], want[1][None])
    assert not torch.equal(wide["a"][0][0], none[0][0]) and not torch.equal(wide["b"][1][0], none[1][0]), "the adapters must change the items"
    release_decoders(m)


# ------------------------------------------------------------------ 4. lifecycle and refusals
def _tiny(dtype=torch.bfloat16):
    dims = synth.LlamaDims(synth.TINY.vocab_size, 256, 1, 4, 512)
    return dims, HipLlama.from_synthetic(dims, 1, dtype=dtype, max_slots=256, max_tokens=256, max_logit_rows=64)


def test_the_17th_adapter_is_refused_and_the_two_kinds_exclude_each_other(lib):
    dims, m = _tiny()
    ad = _adapter(dims, 3)
    for i in range(_lib.LORA_MAX_ADAPTERS):
        m.add_lora(ad, f"n{i}")
    assert sorted(m.adapters.values()) == list(range(1, 17)) and lib.atspeed_llama_lora_slots(m._handle) == 16
    with pytest.raises(_lib.AtSpeedError) as e:
        m.add_lora(ad, "one too many")
    assert e.value.status == _lib.ERR_CAPACITY and "one too many" not in m.adapters and lib.atspeed_llama_lora_slots(m._handle) == 16
    with pytest.raises(ValueError):
        m.add_lora(ad, "n3")
    with pytest.raises(_lib.AtSpeedError) as e:
        m.load_lora(ad)
    assert e.value.status == _lib.ERR_INVALID and m.lora is None
    m.remove_lora("n3")
    assert m.add_lora(ad, "again").adapters["again"] == 4                  # the freed slot is taken again
    for name in list(m.adapters):
        m.remove_lora(name)
    assert lib.atspeed_llama_lora_slots(m._handle) == 0 and lib.atspeed_llama_remove_lora(m._handle, 2) == _lib.ERR_INVALID
    m.load_lora(ad)
    with pytest.raises(_lib.AtSpeedError) as e:
        m.add_lora(ad, "x")
    assert e.value.status == _lib.ERR_INVALID and m.adapters == {}
    assert lib.atspeed_llama_lora_slots(None) == -1


def test_a_decoder_that_names_a_removed_slot_is_refused_before_any_launch(world):
    w = world
    m, fn = w["multi"], w["ci"]["fn"]
    m.add_lora(w["ads"]["a"], "gone")
    slot = m.adapters["gone"]
    m._resident_remove(slot)                           # the library's slot goes, the name stays: the next call names a stale slot
    try:
        m.lora_launches(reset=True)
        with pytest.raises(_lib.AtSpeedError) as e:
            target_generate(m, w["inputs"][1], 4, prefix_allowed_tokens_fn=fn, adapter="gone")
        assert e.value.status == _lib.ERR_INVALID and f"slot {slot}" in e.value.message
        with pytest.raises(_lib.AtSpeedError) as e:
            BSSD_batch(m, w["drf"], w["inputs"][:2], *w["a"], prefix_allowed_tokens_fn=fn, adapters=[None, "gone"])
        assert e.value.status == _lib.ERR_INVALID
        assert m.lora_launches() == 0
    finally:
        del m.adapters["gone"], m.adapter_info["gone"]
    ok = target_generate(m, w["inputs"][1], 4, prefix_allowed_tokens_fn=fn)      # the decoder is usable again once it names a slot that exists
    assert ok["beam_sequence"].shape[0] == w["case"]["K"]
    release_decoders(m, w["drf"])


def test_after_the_last_slot_is_removed_the_model_is_what_it_was():
    """tests/test_lora_gpu.py's unload test for resident slots: with a slot occupied -- even when no sequence names it -- the side path's
    launches run and RoPE is not fused; after the last remove_lora the logits are bit-identical to a model that never had an adapter and the
    fused-RoPE counter advances again"""
    V = synth.BEAUTY.vocab_size
    dims = synth.LlamaDims(V, 1024, 2, 8, 2816)
    make = lambda: HipLlama.from_synthetic(dims, 7, std=0.03, head_std=0.1, dtype=torch.bfloat16, **KW)
    never, m = make(), make()
    g = torch.Generator().manual_seed(4)
    seqs = []
    for i in range(16):
        P, B = 60 + 4 * (i % 8), 40
        T = P + B
        ids = torch.cat((torch.randint(3, 32000, (P,), generator=g), torch.randint(32000, V, (B,), generator=g))).to(torch.int32)
        vis = torch.zeros(T, T, dtype=torch.bool)
        vis[:P, :P] = torch.tril(torch.ones(P, P, dtype=torch.bool))
        vis[P:, :P] = True
        vis[P:, P:] = torch.eye(B, dtype=torch.bool)
        vis[P:, 3 + i % 8] = False
        pos = torch.cat((torch.arange(P), torch.full((B,), P))).to(torch.int32)
        seqs.append((ids, pos, torch.arange(T, dtype=torch.int32), vis_bits_from_bool(vis, 512), T, 4))
    want = never.forward_raw_batch(seqs, return_all=True).clone()
    assert never.rope_fused_launches(reset=True) == dims.n_layers
    m.add_lora(_adapter(dims, 80), "a").add_lora(_adapter(dims, 81, r=16, modules=("q", "k", "v")), "b")
    m.rope_fused_launches(reset=True), m.lora_launches(reset=True)
    unnamed = m.forward_raw_batch(seqs, return_all=True).clone()
    assert m.lora_launches(reset=True) == 2 * dims.n_layers and m.rope_fused_launches() == 0
    # nobody names a slot: the same model through another launch sequence (plain store + RoPE pass).  Each run is within the 16-bit bar of
    # tests/test_fulldims_gpu.py (max 0.04, mean 0.006 of max |logit|) of the exact logits, so the two are within twice that of each other
    scale = float(want.abs().max())
    assert float((unnamed - want).abs().max()) < 2 * 0.04 * scale and float((unnamed - want).abs().mean()) < 2 * 0.006 * scale
    named = m.forward_raw_batch(seqs, return_all=True, adapters=["a", "b"] * 8).clone()
    assert float((named - want).abs().max()) > 0.05 * float(want.abs().max())
    m.remove_lora("a")
    m.lora_launches(reset=True)
    assert m.forward_raw_batch(seqs, return_all=True).shape == want.shape and m.lora_launches(reset=True) == 2 * dims.n_layers
    m.remove_lora("b")
    m.rope_fused_launches(reset=True)
    assert_same("after the last remove_lora vs a model that never had an adapter", m.forward_raw_batch(seqs, return_all=True), want)
    assert m.lora_launches() == 0 and m.rope_fused_launches() == dims.n_layers and m.adapters == {}
