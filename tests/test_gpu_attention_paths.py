"""The attention kernels per kernel, split geometry, page map, mask edge, output writer and scratch
reuse, through `ops.attention_launch`, which sets a launch up as the engine's attnArgs does (page
table, single-row split geometry, f16 / Q80 writers, pinned head group, strides, reused scratch) and
names the kernel instance by the launchers' own predicates (csrc/hip/ops.h attentionLaunch).

Kernels: attnKernel<HG,HS,bf16|f32> (VALU decode, attnTask), attnDecodeMfmaKernel<KM>,
attnPrefillDmaKernel<KM>, attnPrefillKernel<HS>, attnPrefillF32Kernel<HS>. test_kernel_coverage_table tables every
compiled instance against a case that reaches it; attnPrefillKernel<128> is unreachable
(attnPrefillDmaSupported takes every bf16, head-size-128, power-of-two-GQA launch first), so
tests/test_gpu_ops.py::test_attention_prefill_mfma runs attnPrefillDmaKernel at head size 128.

Metric: the largest norm-relative error over every (row, head) slice against float64 attention on the
values the cache stores. Bounds (the project's figures, test_gpu_ops.py; never fitted to a kernel):
    VALU decode 1e-4, f32 prefill 1e-5, bf16 MFMA kernels (decode, both bf16 prefill kernels) 1.2e-2.

Inputs. Every variant carries all of: Gaussian K / V and q = s * Gaussian + a per-KV-head offset (s = 2,
as test_gpu_ops.py, for the f32-arithmetic kernels, 1 for the bf16 MFMA kernels: see _base; the offset so
every head of a group has a positive product with the group's mean q); *poison* at every cache
position no row may read (after the largest position of the slot's rows, unaddressed slots, the
poison page): K = alpha * (the group's mean q), alpha such that its score exceeds every valid score
of every row and head by >= 20 (asserted after bf16 rounding), V = 1024; and, per edge position t, a
*spotlight* variant where key t carries that dominant K and a distinctive V: a kernel that reads one
poisoned key or drops key t is wrong by orders of magnitude more than any bound. Edges: 0, pos, every
chunk's first / last key from the plan (decode rows: attnSplit; prefill row blocks: attnPrefillSplit),
32-key tile edges counted from each chunk's first key (the MFMA decode kernel tiles from c * ch, and ch
is a multiple of 16 only; prefill chunks are whole tiles, so their tile edges are multiples of 32),
128-key round edges from each chunk's first key (VALU), page edges; prefill rows also pos[r] + 1 of
every row (the causal mask inside a block).

The reference path itself, emulated in torch on the CPU over these inputs (test_emulation_*): float64
attention with Q * scale and P rounded to bf16 for the MFMA kernels, float32 attention with a
128-key chunked online softmax for the others; its worst (row, head) error must stay under half the
bound. Worst (row, head) values, CPU emulation | kernel measured on an MI355X:
    VALU decode attnKernel (bound 1e-4):          6.8e-7 | 6.5e-7
    f32 prefill attnPrefillF32Kernel (1e-5):      6.6e-7 | 1.9e-6
    MFMA decode attnDecodeMfmaKernel (1.2e-2):    4.5e-3 | 5.0e-3
    bf16 prefill attnPrefillDmaKernel (1.2e-2):   5.8e-3 | 5.3e-3
    bf16 prefill attnPrefillKernel<64> (1.2e-2):  5.8e-3 | 4.5e-3
(the prefill emulation figure is over both bf16 prefill kernels' cases together).

No length in 1..2048 makes attnSplit's nSplit come out below its first `ns` at the default chunkMin
of 256 (the rounding of ch to 16 would need ns * 15 >= ch); test_split_literals scans them all and
would name one if the rule changed.
"""
import functools

import pytest
import torch

import kernel_checks

gpu = pytest.mark.gpu

B_VALU, B_F32PF, B_MFMA = 1e-4, 1e-5, 1.2e-2
MARGIN = 20.0
LENS = [1, 16, 17, 127, 128, 129, 255, 256, 257, 383, 385, 511, 512, 513, 1024, 1025]
TILE_LENS = [31, 32, 33, 63, 64, 65]


@pytest.fixture(scope="module")
def ops():
    return _ops()


def _ops():
    from distributed_llama_multiusers_amd import ops as o
    return o


def bf16(x):
    return x.bfloat16().to(x.dtype)


def head_rel(got, want, hs):
    """Largest norm-relative error over the (row, head) slices: one wrong head cannot hide."""
    g, w = got.double().reshape(got.shape[0], -1, hs), want.double().reshape(got.shape[0], -1, hs)
    return float(((g - w).norm(dim=-1) / w.norm(dim=-1).clamp_min(1e-30)).max())


def check(name, got, want, hs, tol):
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: unwritten or non-finite elements"
    r = head_rel(got, want, hs)
    print(f"{name}: worst (row, head) rel {r:.3e} (bound {tol:.1e})")
    assert r < tol, (name, r, tol)
    return r


# ------------------------------------------------------------------------------------------ cases
class Case:
    def __init__(self, name, pos, slots=None, n_slots=None, H=None, kvm=1, hs=128, seq=2048, bf=True, seed=7, **launch):
        self.name, self.pos, self.kvm, self.hs, self.seq, self.bf, self.seed = name, list(pos), kvm, hs, seq, bf, seed
        self.H = H if H is not None else kvm
        self.slots = list(slots) if slots is not None else list(range(len(pos)))[::-1]
        self.n_slots = n_slots if n_slots is not None else max(self.slots) + 2  # one slot no row addresses
        self.launch = launch
        self.prefill = bool(launch.get("prefill"))

    @property
    def bound(self):
        """by the kernel the plan names: bf16 MFMA kernels, the f32 prefill kernel, else the VALU kernel."""
        if not hasattr(self, "_bound"):
            k = plan_of(self)["kernel"]
            mfma = k.startswith(("attnDecodeMfmaKernel", "attnPrefillDmaKernel", "attnPrefillKernel"))
            self._bound = B_MFMA if mfma else B_F32PF if k.startswith("attnPrefillF32Kernel") else B_VALU
        return self._bound

    def last(self):
        """per slot: the largest position of the rows that address it (-1: none)."""
        last = [-1] * self.n_slots
        for p, s in zip(self.pos, self.slots):
            last[s] = max(last[s], p)
        return last


SPOT_V = lambda kv0: ((torch.arange(kv0) % 13) - 6).float()  # noqa: E731  (integers: exact in bf16)


@functools.lru_cache(maxsize=8)
def _base(c):
    """Gaussian + poison operands of a case: (q [B, q0], k, v [slots, seq, kv0], poison K row, poison V row)."""
    g = torch.Generator().manual_seed(c.seed)
    B, nkv = len(c.pos), c.H // c.kvm
    kv0 = nkv * c.hs
    k = torch.randn(c.n_slots, c.seq, kv0, generator=g)
    v = torch.randn(c.n_slots, c.seq, kv0, generator=g)
    mu = torch.randn(nkv, c.hs, generator=g)
    # the q scale of test_gpu_ops.py (2) where the arithmetic is f32; 1 for the bf16 MFMA kernels, whose
    # reference path (emulate) misses half of 1.2e-2 at scale 2 on rows of a few keys (6.6e-3 at len 16..31)
    rounds = c.bf and (c.prefill or c.launch.get("kernel", "auto") != "valu")
    q = torch.randn(B, nkv, c.kvm, c.hs, generator=g) * (1 if rounds else 2) + mu[None, :, None, :]
    if c.bf:
        k, v = bf16(k), bf16(v)
    mq = q.mean((0, 2))  # [nkv, hs]
    kd, qd = k.double().reshape(c.n_slots, c.seq, nkv, c.hs), q.double()
    smax = torch.full((nkv,), -1e30, dtype=torch.float64)
    for b, (p, s) in enumerate(zip(c.pos, c.slots)):
        sc = torch.einsum("tkd,kmd->kmt", kd[s, :p + 1], qd[b]) / c.hs ** 0.5
        smax = torch.maximum(smax, sc.amax((1, 2)))
    dots = torch.einsum("bkmd,kd->bkm", qd, mq.double()) / c.hs ** 0.5
    dmin = dots.amin((0, 2))
    assert bool((dmin > 0).all()), "a head has no positive product with its group's mean q"
    alpha = (smax + MARGIN + 2.0) / dmin
    pk = (alpha[:, None] * mq.double()).float()
    if c.bf:
        pk = bf16(pk)
    margin = torch.einsum("bkmd,kd->bkm", qd, pk.double()) / c.hs ** 0.5 - smax[None, :, None]
    assert float(margin.min()) >= MARGIN, float(margin.min())
    pk, pv = pk.reshape(-1), torch.full((kv0,), 1024.0)
    for s, last in enumerate(c.last()):
        k[s, last + 1:] = pk
        v[s, last + 1:] = pv
    return q.reshape(B, -1), k, v, pk, pv


def operands(c, spot=None):
    q, k, v, pk, pv = _base(c)
    if spot is not None:
        k, v = k.clone(), v.clone()
        for s, last in enumerate(c.last()):
            if spot <= last:
                k[s, spot] = pk
                v[s, spot] = SPOT_V(v.shape[-1])
    return q, k, v, pk, pv


def reference(c, q, k, v):
    return _ops().ref_attention(q, k, v, c.H, c.kvm, c.hs, c.pos, c.slots, dtype=torch.float64)


def plan_of(c, **kw):
    q, k, v, _, _ = _base(c)
    return _ops().attention_launch(q, k, v, c.H, c.kvm, c.hs, c.pos, c.slots, c.bf, plan_only=True, **{**c.launch, **kw})


def spots(c, page=0, **kw):
    """The edge positions of a case (see the header), those some row can see."""
    p = plan_of(c, **kw)
    top = max(c.pos)
    e = {0, *c.pos}
    if c.prefill:
        e |= {x + 1 for x in c.pos}
        rpb = 64 // c.kvm
        tops = [max(c.pos[b0:b0 + rpb]) for b0 in range(0, len(c.pos), rpb)]
        lows = [min(c.pos[b0:b0 + rpb]) for b0 in range(0, len(c.pos), rpb)]
    else:
        tops = lows = c.pos
    step = 128 if p["kernel"].startswith("attnKernel") else 32
    for (ns, ch), hi, lo in zip(p["splits"], tops, lows):
        for i in range(ns):
            if i:
                e |= {i * ch - 1, i * ch}  # the chunk's edge
            for t in range(i * ch + step, min((i + 1) * ch, hi + 1), step):
                if c.prefill and t < lo - 64:
                    continue  # deep below every row of the block: the chunk edges only, every tile edge near the rows
                e |= {t - 1, t}
    if page:
        for t in range(page, top + 1, page):
            e |= {t - 1, t}
    return sorted(t for t in e if 0 <= t <= top)


def launch(ops, c, q, k, v, pk, pv, **kw):
    return ops.attention_launch(q, k, v, c.H, c.kvm, c.hs, c.pos, c.slots, c.bf, poison_k=pk, poison_v=pv,
                                **{**c.launch, **kw})


def verify(ops, c, kernel_prefix, page=0, page_of=None, spot_list=None, **kw):
    """Gaussian + poison, then every spotlight variant: the reference check on each, the kernel named
    by the plan; with a page map also bitwise equality with the same launch on a contiguous cache."""
    worst = 0.0
    for t in [None] + (spots(c, page, **kw) if spot_list is None else spot_list):
        q, k, v, pk, pv = operands(c, t)
        r = launch(ops, c, q, k, v, pk, pv, **kw)
        assert r["kernel"].startswith(kernel_prefix), (r["kernel"], kernel_prefix)
        want = reference(c, q, k, v)
        worst = max(worst, check(f"{c.name} {r['kernel']} spot {t}", r["out"], want, c.hs, c.bound))
        if page:
            rp = launch(ops, c, q, k, v, pk, pv, page_size=page, page_of=page_of, **kw)
            assert rp["kernel"] == r["kernel"]
            assert torch.equal(rp["out"], r["out"]), f"{c.name} spot {t}: paged != contiguous, bitwise"
    print(f"{c.name}: worst over variants {worst:.3e}")
    return worst


def page_map(c, page):
    """A fixed permutation, neither identity nor monotone, the slots' pages interleaved; only the
    pages the rows reach are mapped (the rest: -1, the poison page)."""
    pps = (c.seq + page - 1) // page
    n = c.n_slots * pps
    po = [[-1] * pps for _ in range(c.n_slots)]
    for s, last in enumerate(c.last()):
        for pg in range(last // page + 1 if last >= 0 else 0):
            po[s][pg] = ((pg * c.n_slots + s) * 7 + 3) % n  # 7 is coprime to every n used here (asserted)
    flat = [x for r in po for x in r if x >= 0]
    assert len(set(flat)) == len(flat), "page map is not a permutation"
    return po


# ------------------------------------------------------------------------------- CPU: the emulations
def emulate(c, q, k, v, mutate=None, ch_of=None):
    """The reference path in torch (not the kernel): bf16 kernels -> float64 attention with Q * scale
    and P rounded to bf16; others -> float32 attention, online softmax over 128-key chunks.
    mutate (the issue's mask / split mutations, evaluated here on the CPU): "t1-1" drops each chunk's
    last key, "t1+1" reads one key past each chunk's end (at the last chunk: key pos + 1), "nocausal"
    drops the per-row term of the prefill mask (every row sees the block's largest position)."""
    mfma = c.bound == B_MFMA
    out = torch.zeros(len(c.pos), c.H * c.hs, dtype=torch.float64)
    top = max(c.pos)
    for b, (p, s) in enumerate(zip(c.pos, c.slots)):
        n = (top if mutate == "nocausal" else p) + 1
        ch = ch_of[b] if ch_of else n
        keys = []
        for t0 in range(0, n, ch):
            t1 = min(t0 + ch, n) + {"t1-1": -1, "t1+1": 1}.get(mutate, 0)
            keys += list(range(t0, min(t1, c.seq)))
        keys = torch.tensor(sorted(set(keys)), dtype=torch.long)
        for h in range(c.H):
            sl = slice(h // c.kvm * c.hs, (h // c.kvm + 1) * c.hs)
            K, V, qh = k[s, keys, sl], v[s, keys, sl], q[b, h * c.hs:(h + 1) * c.hs]
            if mfma:
                sc = K.double() @ bf16(qh / c.hs ** 0.5).double()
                pr = torch.exp(sc - sc.max())
                o = bf16(pr.float()).double() @ V.double() / pr.sum()
            else:
                m, l, acc = torch.tensor(-float("inf")), torch.tensor(0.0), torch.zeros(c.hs)
                qs = (qh / c.hs ** 0.5).float()
                for i in range(0, len(keys), 128):
                    sc = K[i:i + 128].float() @ qs
                    mn = torch.maximum(m, sc.max())
                    pr = torch.exp(sc - mn)
                    l, acc, m = l * torch.exp(m - mn) + pr.sum(), acc * torch.exp(m - mn) + pr @ V[i:i + 128].float(), mn
                o = (acc / l).double()
            out[b, h * c.hs:(h + 1) * c.hs] = o
    return out


def split_cases(bf, hs, single):
    if single:
        return [Case(f"single len{n} bf{int(bf)} hs{hs}", [n - 1], hs=hs, bf=bf, kernel="valu", single=True) for n in LENS]
    return [Case(f"batched lens{LENS[i:i + 3]} bf{int(bf)} hs{hs}", [n - 1 for n in LENS[i:i + 3]], hs=hs, bf=bf,
                 kernel="valu") for i in range(0, len(LENS), 3)]


def mfma_cases(kvm, single):
    lens = sorted(LENS + TILE_LENS)
    if single:
        return [Case(f"mfma single len{n} kvm{kvm}", [n - 1], kvm=kvm, kernel="mfma", single=True) for n in lens]
    return [Case(f"mfma batched lens{lens[i:i + 4]} kvm{kvm}", [n - 1 for n in lens[i:i + 4]], kvm=kvm, kernel="mfma")
            for i in range(0, len(lens), 4)]


def prefill_cases():
    cs = []
    for kvm in (1, 2, 4, 8, 16):  # DMA kernel; 64 / kvm rows per block
        rpb = 64 // kvm
        # two blocks in different slots, the second partial; the first from position 0; rows straddle tile 32
        n2 = max(1, rpb // 2 - 1)
        cs.append(Case(f"dma kvm{kvm} two blocks", list(range(rpb)) + list(range(300, 300 + n2)),
                       slots=[1] * rpb + [0] * n2, n_slots=3, kvm=kvm, seq=512, prefill=True))
    # maxLen 266 -> attnPrefillSplit gives 2 chunks of 160 keys (asserted in test_split_literals): rows
    # 150..165 lie on both sides of the chunk edge, rows below it are fully masked in chunk 1
    cs.append(Case("dma kvm4 straddle split", list(range(150, 165)) + [265], slots=[0] * 16, n_slots=2, kvm=4, seq=512,
                   prefill=True))
    # non-consecutive positions inside a block
    cs.append(Case("dma kvm8 scattered", [5, 40, 41, 100, 31, 32, 260], slots=[1] * 7, n_slots=2, kvm=8, seq=512, prefill=True))
    cs.append(Case("pf bf16 hs64 two blocks", list(range(16)) + list(range(250, 262)), slots=[1] * 16 + [0] * 12,
                   n_slots=3, kvm=4, hs=64, seq=512, prefill=True))
    cs.append(Case("pf bf16 hs64 scattered", [5, 40, 41, 100, 31, 32, 260], slots=[0] * 7, n_slots=2, kvm=8, hs=64,
                   seq=512, prefill=True))
    for hs in (64, 128):
        cs.append(Case(f"pf f32 hs{hs} two blocks", list(range(16)) + list(range(120, 132)), slots=[1] * 16 + [0] * 12,
                       n_slots=3, kvm=4, hs=hs, seq=512, bf=False, prefill=True))
        cs.append(Case(f"pf f32 hs{hs} scattered", [5, 40, 41, 100, 31, 32, 260], slots=[0] * 7, n_slots=2, kvm=8,
                       hs=hs, seq=512, bf=False, prefill=True))
    return cs


def hg_cases():
    cs = [Case(f"hg{hg} kvm8", [300, 17, 600], kvm=8, H=8, kernel="valu", head_group=hg) for hg in (1, 2, 4, 8)]
    cs.append(Case("hg1 kvm4", [300, 17, 600], kvm=4, H=4, kernel="valu", head_group=1))
    return cs


def all_cases():
    cs = []
    for bf in (True, False):
        for hs in (128, 64):
            cs += split_cases(bf, hs, True) + split_cases(bf, hs, False)
    for kvm in (1, 2, 4, 8):
        cs += mfma_cases(kvm, True) + mfma_cases(kvm, False)
    return cs + prefill_cases() + hg_cases()


@pytest.mark.parametrize("family", ["valu", "mfma", "prefill"])
def test_emulation_under_half_bound(family):
    """CPU: the reference path's own error over the suite's inputs (Gaussian + poison, and the first,
    a middle and the last spotlight of every case) stays under half of each bound."""
    worst = {}
    for c in all_cases():
        fam = "prefill" if c.prefill else ("mfma" if c.bound == B_MFMA else "valu")
        if fam != family:
            continue
        e = spots(c)
        for t in [None, e[0], e[len(e) // 2], e[-1]]:
            q, k, v, _, _ = operands(c, t)
            r = head_rel(emulate(c, q, k, v), reference(c, q, k, v), c.hs)
            worst[c.bound] = max(worst.get(c.bound, 0.0), r)
            assert r < c.bound / 2, (c.name, t, r)
    print(f"{family}: worst emulated (row, head) error per bound {worst}")


def test_mutations_are_caught_by_the_emulation():
    """CPU: the mask / split mutations of attnTask and of the prefill mask, evaluated in the emulation
    on the suite's inputs, miss the bound by far on a variant the GPU tests run."""
    c = Case("single len385", [384], kernel="valu", single=True)
    ns, ch = plan_of(c)["splits"][0]
    assert ns > 1
    q, k, v, _, _ = operands(c, ch - 1)  # the first chunk's last key, spotlit
    assert head_rel(emulate(c, q, k, v, "t1-1", [ch]), reference(c, q, k, v), c.hs) > 100 * c.bound
    q, k, v, _, _ = operands(c, None)    # key pos + 1 is poison
    assert head_rel(emulate(c, q, k, v, "t1+1", [ch]), reference(c, q, k, v), c.hs) > 100 * c.bound
    assert head_rel(emulate(c, q, k, v, None, [ch]), reference(c, q, k, v), c.hs) < c.bound / 2
    p = Case("dma kvm8 scattered", [5, 40, 41, 100, 31, 32, 260], slots=[1] * 7, n_slots=2, kvm=8, seq=512, prefill=True)
    q, k, v, _, _ = operands(p, 6)       # key pos[0] + 1: must not touch row 0
    assert head_rel(emulate(p, q, k, v, "nocausal"), reference(p, q, k, v), p.hs) > 100 * p.bound


# ------------------------------------------------------------------- CPU: plan, literals, refusals
# (nSplit, ch) of attnSplit for len = LENS, derived by hand from the rule (chunkMin 256; rows of <= 512
# keys in single mode: 128; ns = ceil(len / chunk) clamped to the grid; ch = ceil(len / ns) rounded up
# to 16; nSplit = ceil(len / ch)). seqLen 2048: grid 8 either way.
SPLITS_SINGLE = {1: (1, 16), 16: (1, 16), 17: (1, 32), 127: (1, 128), 128: (1, 128), 129: (2, 80), 255: (2, 128),
                 256: (2, 128), 257: (3, 96), 383: (3, 128), 385: (4, 112), 511: (4, 128), 512: (4, 128),
                 513: (3, 176), 1024: (4, 256), 1025: (5, 208)}
SPLITS_BATCHED = {1: (1, 16), 16: (1, 16), 17: (1, 32), 127: (1, 128), 128: (1, 128), 129: (1, 144), 255: (1, 256),
                  256: (1, 256), 257: (2, 144), 383: (2, 192), 385: (2, 208), 511: (2, 256), 512: (2, 256),
                  513: (3, 176), 1024: (4, 256), 1025: (5, 208)}


def test_split_literals():
    for single, table in ((True, SPLITS_SINGLE), (False, SPLITS_BATCHED)):
        c = Case("lens", [n - 1 for n in LENS], slots=[0] * len(LENS), hs=64, kernel="valu", single=single)
        p = plan_of(c)
        assert p["split_grid"] == 8 and p["short_len"] == (512 if single else 0) and p["chunk_max"] == 272
        assert [tuple(x) for x in p["splits"]] == [table[n] for n in LENS]
        # every length: the chunks tile [0, len) with no empty chunk, within the grid; none has nSplit
        # below the first ns (see the header)
        c = Case("all", list(range(2048)), slots=[0] * 2048, hs=64, kernel="valu", single=single)
        for n, (ns, ch) in enumerate(plan_of(c)["splits"], 1):
            chunk = 128 if single and n <= 512 else 256
            assert ch % 16 == 0 and (ns - 1) * ch < n <= ns * ch and ns <= 8
            assert ns == min(8, -(-n // chunk)), f"len {n}: nSplit {ns} below the first ns: add it to LENS"
    # prefill row blocks (attnPrefillSplit): ~256 keys per chunk (128: the f32 kernel on a small grid), whole 32-key tiles
    straddle = [c for c in prefill_cases() if c.name == "dma kvm4 straddle split"][0]
    assert plan_of(straddle)["splits"] == [(2, 160)]
    two = Case("pf", list(range(16)) + list(range(250, 262)), slots=[1] * 16 + [0] * 12, n_slots=3, kvm=4, hs=64, seq=512, prefill=True)
    assert plan_of(two)["splits"] == [(1, 32), (2, 160)]
    f32 = Case("pf", list(range(120, 132)), slots=[1] * 12, n_slots=2, kvm=4, hs=64, seq=512, bf=False, prefill=True)
    assert plan_of(f32)["splits"] == [(2, 96)]
    # a forced grid of 2 at len 1000: ns clamped, ch above chunkMin
    c = Case("forced", [999], kernel="valu", split_grid=2)
    assert plan_of(c)["splits"] == [(2, 512)] and plan_of(c)["chunk_max"] == 1040


# instance -> (case that reaches it, the launch's own keywords); None: unreachable, with the reason
def _cov():
    cov = {}
    for hs in (64, 128):
        for bf in (True, False):
            for hg in (1, 2, 4, 8):
                cov[f"attnKernel<{hg},{hs},{'bf16' if bf else 'f32'}>"] = Case(
                    "cov", [300, 17, 600], kvm=8, H=8, hs=hs, bf=bf, kernel="valu", head_group=hg)
        cov[f"attnPrefillF32Kernel<{hs}>"] = Case("cov", [3, 4], slots=[0, 0], kvm=4, hs=hs, bf=False, seq=512, prefill=True)
    for km in (1, 2, 4, 8):
        cov[f"attnDecodeMfmaKernel<{km}>"] = Case("cov", [100], kvm=km, kernel="mfma")
    for km in (1, 2, 4, 8, 16):
        cov[f"attnPrefillDmaKernel<{km}>"] = Case("cov", [3, 4], slots=[0, 0], kvm=km, seq=512, prefill=True)
    cov["attnPrefillKernel<64>"] = Case("cov", [3, 4], slots=[0, 0], kvm=4, hs=64, seq=512, prefill=True)
    cov["attnPrefillKernel<128>"] = None  # shadowed: attnPrefillDmaSupported (bf16, hs 128, kvMul 1..16 power of two)
    return cov


# every attention instance the launchers can name (kernels.hip attnDispatchHG, attn_mfma.hip
# DL_AM_CASE / DL_AP_CASE, attn_prefill.hip launchAttentionPrefill)
INSTANCES = ([f"attnKernel<{hg},{hs},{t}>" for hg in (1, 2, 4, 8) for hs in (64, 128) for t in ("bf16", "f32")]
             + [f"attnDecodeMfmaKernel<{k}>" for k in (1, 2, 4, 8)] + [f"attnPrefillDmaKernel<{k}>" for k in (1, 2, 4, 8, 16)]
             + [f"attnPrefillKernel<{h}>" for h in (64, 128)] + [f"attnPrefillF32Kernel<{h}>" for h in (64, 128)])


def test_kernel_coverage_table():
    cov = _cov()
    assert sorted(cov) == sorted(INSTANCES)
    for name, c in cov.items():
        if c is not None:
            assert plan_of(c)["kernel"] == name
    # the shadowed instance: every bf16 head-size-128 prefill launch the launcher accepts goes to the DMA kernel
    for km in (1, 2, 4, 8, 16):
        c = Case("shadow", [3, 4], slots=[0, 0], kvm=km, seq=512, prefill=True)
        assert plan_of(c)["kernel"] == f"attnPrefillDmaKernel<{km}>"


@gpu
@pytest.mark.parametrize("name", [n for n in INSTANCES if n != "attnPrefillKernel<128>"])
def test_every_reachable_instance_runs(ops, name):
    """The coverage table's case of every reachable instance, launched: the kernel the launch reports
    is that instance, and it meets its bound (Gaussian + poison, spotlights at 0, a chunk edge and pos)."""
    c = _cov()[name]
    e = spots(c)
    q, k, v, pk, pv = operands(c)
    assert launch(ops, c, q, k, v, pk, pv)["kernel"] == name
    verify(ops, c, name, spot_list=[e[0], e[len(e) // 2], e[-1]])


def test_auto_picks_mfma_exactly_when_supported_and_long():
    for bf, hs, kvm, seq, want in [(True, 128, 4, 1024, "attnDecodeMfmaKernel<4>"), (True, 128, 4, 1008, "attnKernel"),
                                   (True, 128, 8, 2048, "attnDecodeMfmaKernel<8>"), (True, 128, 16, 2048, "attnKernel"),
                                   (True, 64, 4, 2048, "attnKernel"), (False, 128, 4, 2048, "attnKernel"),
                                   (True, 128, 1, 1024, "attnDecodeMfmaKernel<1>"), (True, 128, 2, 1024, "attnDecodeMfmaKernel<2>")]:
        c = Case("auto", [5], kvm=kvm, hs=hs, bf=bf, seq=seq)
        assert plan_of(c)["kernel"].startswith(want), (bf, hs, kvm, seq, plan_of(c)["kernel"])


def test_head_group_pick():
    # 8 heads x 8 splits x 3 rows = 192 workgroups <= 256: one head each; 5 rows = 320: two; 32 heads x 8 x 4: eight
    assert plan_of(Case("hg", [9] * 3, kvm=8, H=8, kernel="valu"))["hg"] == 1
    assert plan_of(Case("hg", [9] * 5, kvm=8, H=8, kernel="valu"))["hg"] == 2
    p = plan_of(Case("hg", [9] * 4, kvm=8, H=32, kernel="valu"))
    assert p["hg"] == 4 and p["kernel"] == "attnKernel<4,128,bf16>" and p["grid"] == (8, 8, 4)
    assert plan_of(Case("hg", [9] * 5, kvm=8, H=8, kernel="valu", head_group=1))["hg"] == 1
    assert plan_of(Case("hg", [9], kvm=4, H=4, kernel="valu", head_group=8))["hg"] == 4


def test_refusals():
    def refused(msg, c, **kw):
        with pytest.raises(RuntimeError, match=msg):
            plan_of(c, **kw)
    one = Case("r", [100], kvm=4)
    pps = lambda c, page: [0] * (c.n_slots * (c.seq // page))  # noqa: E731
    refused("more than 64 pages", one, kernel="mfma", split_grid=1, page_size=32, page_of=pps(one, 32))
    long = Case("r", [3, 4], slots=[0, 0], kvm=4, seq=8192 * 2, prefill=True)
    refused("paged context too long", long, split_grid=1, page_size=32, page_of=pps(long, 32))
    long64 = Case("r", [3, 4], slots=[0, 0], kvm=4, hs=64, seq=8192 * 2, prefill=True)
    refused("paged context too long", long64, split_grid=1, page_size=32, page_of=pps(long64, 32))
    refused("MFMA decode attention", Case("r", [5], kvm=16), kernel="mfma")
    refused("MFMA decode attention", Case("r", [5], kvm=4, hs=64), kernel="mfma")
    refused("power-of-two GQA", Case("r", [5], kvm=3, H=3, hs=64, prefill=True))
    refused("share a slot", Case("r", [3, 4], slots=[0, 1], kvm=4, seq=512, prefill=True))
    refused("ignore outQ", Case("r", [3, 4], slots=[0, 0], kvm=4, seq=512, prefill=True), out="q80")
    refused("headGroup", one, kernel="valu", head_group=3)
    refused("pageSize", one, page_size=16, page_of=[0])
    refused("pageOf", one, page_size=64, page_of=[0])
    refused("ldOut", one, ld_out=one.H * one.hs + 8)
    refused("repeat", one, repeat=0)


# --------------------------------------------------------------------------------------- GPU: cases
@gpu
@pytest.mark.parametrize("single", [True, False])
@pytest.mark.parametrize("hs", [128, 64])
@pytest.mark.parametrize("bf", [True, False])
def test_valu_split_geometry(ops, bf, hs, single):
    """Case 1: the VALU decode kernel over LENS, single-row (shortLen 512, chunks of 128) and batched
    (3 rows of different lengths, reversed slots) geometry."""
    for c in split_cases(bf, hs, single):
        verify(ops, c, f"attnKernel<1,{hs},")


@gpu
def test_valu_forced_split_grid(ops):
    c = Case("forced grid 2 len1000", [999], kernel="valu", split_grid=2)
    assert plan_of(c)["splits"] == [(2, 512)]
    verify(ops, c, "attnKernel<1,128,bf16>")


@gpu
@pytest.mark.parametrize("single", [True, False])
@pytest.mark.parametrize("kvm", [1, 2, 4, 8])
def test_mfma_decode(ops, kvm, single):
    """Case 2: the MFMA decode kernel over LENS and the 32-key tile edges, every GQA group size."""
    for c in mfma_cases(kvm, single):
        verify(ops, c, f"attnDecodeMfmaKernel<{kvm}>")


@gpu
def test_auto_runs_mfma_at_1024(ops):
    c = Case("auto seq1024", [700, 31], kvm=4, seq=1024)
    verify(ops, c, "attnDecodeMfmaKernel<4>")


@gpu
def test_head_groups(ops):
    """Case 3: every HG within the VALU bound; headGroup 1 bitwise the same alone or among other rows."""
    for c in hg_cases():
        verify(ops, c, f"attnKernel<{c.launch['head_group']},128,bf16>")
    big = Case("hg auto", [300, 17, 600, 5, 129], kvm=8, H=8, kernel="valu")
    assert plan_of(big)["hg"] == 2
    verify(ops, big, "attnKernel<2,128,bf16>", spot_list=[0, 128, 300])
    c = hg_cases()[0]
    q, k, v, pk, pv = operands(c)
    both = launch(ops, c, q, k, v, pk, pv)["out"]
    for b in range(len(c.pos)):
        alone = ops.attention_launch(q[b:b + 1], k, v, c.H, c.kvm, c.hs, c.pos[b:b + 1], c.slots[b:b + 1], c.bf,
                                     kernel="valu", head_group=1)["out"]
        assert torch.equal(alone[0], both[b]), f"row {b}: headGroup 1 differs between a launch alone and among rows"


@gpu
@pytest.mark.parametrize("i", range(len(prefill_cases())))
def test_prefill(ops, i):
    """Case 4: DMA (hs 128, kvMul 1..16), register-staged bf16 (hs 64) and f32 (hs 64 / 128) prefill."""
    c = prefill_cases()[i]
    verify(ops, c, "attnPrefill")


PAGED = [Case("paged valu", [300, 17, 600], kvm=2, kernel="valu"),
         Case("paged valu single f32 hs64", [400], kvm=2, hs=64, bf=False, kernel="valu", single=True),
         Case("paged mfma", [300, 17, 600], kvm=2, kernel="mfma"),
         Case("paged mfma single", [400], kvm=4, kernel="mfma", single=True),
         Case("paged dma", list(range(250, 266)), slots=[0] * 16, n_slots=2, kvm=4, seq=512, prefill=True),
         Case("paged pf hs64", list(range(250, 262)), slots=[1] * 12, n_slots=2, kvm=4, hs=64, seq=512, prefill=True),
         Case("paged pf f32", list(range(120, 132)), slots=[1] * 12, n_slots=2, kvm=4, hs=128, seq=512, bf=False, prefill=True),
         # two row blocks in two slots, their pages interleaved
         Case("paged dma two slots", list(range(100, 116)) + list(range(250, 262)), slots=[1] * 16 + [0] * 12, n_slots=3,
              kvm=4, seq=512, prefill=True),
         Case("paged pf hs64 two slots", list(range(100, 116)) + list(range(250, 262)), slots=[1] * 16 + [0] * 12, n_slots=3,
              kvm=4, hs=64, seq=512, prefill=True)]


@gpu
@pytest.mark.parametrize("page", [32, 64, 256])
@pytest.mark.parametrize("i", range(len(PAGED)))
def test_paged(ops, i, page):
    """Case 5: a permuted, interleaved page map with a partly used last page per slot: bitwise equal
    to the contiguous launch, and within the bound."""
    c = PAGED[i]
    verify(ops, c, "attn", page=page, page_of=page_map(c, page))


@gpu
def test_paged_mfma_chunk_of_many_pages(ops):
    c = Case("paged mfma 32 pages per chunk", [999], kvm=2, seq=1024, kernel="mfma", split_grid=1)
    assert plan_of(c)["splits"] == [(1, 1008)]
    verify(ops, c, "attnDecodeMfmaKernel<2>", page=32, page_of=page_map(c, 32), spot_list=[0, 31, 32, 511, 512, 991, 992, 999])


OUT_CASES = [Case("out valu", [300, 17, 600], kvm=8, H=8, kernel="valu"),
             Case("out valu f32 hs64", [300, 17], kvm=2, hs=64, bf=False, kernel="valu"),
             Case("out mfma", [300, 17, 600], kvm=4, kernel="mfma"),
             Case("out dma", list(range(250, 266)), slots=[0] * 16, n_slots=2, kvm=4, seq=512, prefill=True),
             Case("out pf hs64", list(range(250, 262)), slots=[1] * 12, n_slots=2, kvm=4, hs=64, seq=512, prefill=True),
             Case("out pf f32", list(range(120, 132)), slots=[1] * 12, n_slots=2, kvm=4, hs=64, seq=512, bf=False, prefill=True)]


@gpu
@pytest.mark.parametrize("i", range(len(OUT_CASES)))
def test_f16_output_is_the_rounded_f32_output(ops, i):
    """Case 6: outH of every kernel = its f32 output rounded to f16, bitwise."""
    c = OUT_CASES[i]
    for t in (None, 0, max(c.pos)):
        q, k, v, pk, pv = operands(c, t)
        f32 = launch(ops, c, q, k, v, pk, pv)["out"]
        f16 = launch(ops, c, q, k, v, pk, pv, out="f16")["out"]
        assert torch.equal(f16, f32.half().float()), (c.name, t)


@gpu
@pytest.mark.parametrize("kernel,hg", [("valu", 1), ("valu", 2), ("valu", 4), ("valu", 8), ("mfma", 0)])
@pytest.mark.parametrize("single", [True, False])
def test_q80_output(ops, kernel, hg, single):
    """Case 6: the Q80 writer (attnWriteOut, direct and behind the combine) at single- and multi-chunk rows."""
    for pos in ([100], [700]):
        c = Case(f"q80 {kernel} hg{hg} pos{pos}", pos, kvm=8, H=8, kernel=kernel, head_group=hg, single=single)
        assert (plan_of(c)["splits"][0][0] > 1) == (pos[0] > 128)
        for t in (None, 0, pos[0]):
            q, k, v, pk, pv = operands(c, t)
            r = launch(ops, c, q, k, v, pk, pv, out="q80")
            want = reference(c, q, k, v)
            kernel_checks.check_q80_row(r["out"].long(), r["scales"][..., 0], r["scales"][..., 1], want,
                              f"{c.name} spot {t}", kernel_bound=c.bound)


@gpu
@pytest.mark.parametrize("hs,bf", [(64, True), (64, False), (128, False)])
@pytest.mark.parametrize("hg", [1, 4])
def test_q80_output_other_instances(ops, hs, bf, hg):
    """The Q80 writer of the hs 64 and f32-cache VALU instances, single- and multi-chunk rows."""
    for pos in ([100], [700]):
        c = Case(f"q80 hs{hs} bf{int(bf)} hg{hg} pos{pos}", pos, kvm=4, H=4, hs=hs, bf=bf, kernel="valu", head_group=hg, single=True)
        for t in (None, pos[0]):
            q, k, v, pk, pv = operands(c, t)
            r = launch(ops, c, q, k, v, pk, pv, out="q80")
            assert r["kernel"] == f"attnKernel<{hg},{hs},{'bf16' if bf else 'f32'}>"
            kernel_checks.check_q80_row(r["out"].long(), r["scales"][..., 0], r["scales"][..., 1], reference(c, q, k, v),
                                        f"{c.name} spot {t}", kernel_bound=c.bound)


REUSE = [(Case("reuse valu", [1500, 700, 900], kvm=2, kernel="valu"), [40, 300, 2]),
         (Case("reuse mfma", [1500, 700, 900], kvm=2, kernel="mfma"), [40, 300, 2]),
         (Case("reuse dma", list(range(400, 416)), slots=[0] * 16, n_slots=2, kvm=4, seq=512, prefill=True), list(range(3, 19))),
         (Case("reuse pf hs64", list(range(400, 416)), slots=[0] * 16, n_slots=2, kvm=4, hs=64, seq=512, prefill=True), list(range(3, 19))),
         (Case("reuse pf f32", list(range(400, 416)), slots=[0] * 16, n_slots=2, kvm=4, hs=64, seq=512, bf=False, prefill=True), list(range(3, 19)))]


@gpu
@pytest.mark.parametrize("i", range(len(REUSE)))
def test_scratch_reuse(ops, i):
    """Case 7: three launches on one scratch (the op asserts bitwise repeats and zeroed counters), then
    the same shapes with shorter rows on the scratch and output buffer the longer rows' launch just
    used (warm_pos): a stale partO / partML slot or counter of the longer run must not leak."""
    c, short = REUSE[i]
    verify(ops, c, "attn", spot_list=[0, max(c.pos)], repeat=3)
    s = Case(c.name + " shorter", short, slots=c.slots, n_slots=c.n_slots, H=c.H, kvm=c.kvm, hs=c.hs, seq=c.seq, bf=c.bf, **c.launch)
    assert max(ns for ns, _ in plan_of(s)["splits"]) < max(ns for ns, _ in plan_of(c)["splits"])
    verify(ops, s, "attn", spot_list=[0, max(short)], repeat=3, warm_pos=c.pos)


@gpu
@pytest.mark.parametrize("i", range(len(OUT_CASES)))
def test_strides_and_guards(ops, i):
    """Case 8: ldq > q0 and ldOut > q0 (guards after every row's valid part)."""
    c = OUT_CASES[i]
    q0 = c.H * c.hs
    for t in (None, max(c.pos)):
        q, k, v, pk, pv = operands(c, t)
        qw = torch.full((q.shape[0], q0 + 36), 1e4)
        qw[:, :q0] = q
        for out in ("f32", "f16") + (() if c.prefill else ("q80",)):
            r = launch(ops, c, qw, k, v, pk, pv, ldq=q0 + 36, ld_out=q0 + 64, out=out)
            same = launch(ops, c, q, k, v, pk, pv, out=out)
            assert torch.equal(r["out"], same["out"]), (c.name, out, t)
        check(f"{c.name} strided spot {t}", launch(ops, c, qw, k, v, pk, pv, ldq=q0 + 36, ld_out=q0 + 64)["out"],
              reference(c, q, k, v), c.hs, c.bound)
