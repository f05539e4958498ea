"""The structured attention inputs of tests/attn_patterns.py, checked on the CPU: the builders keep their own claims,
the fp64 softmax of each pattern meets its comparator, the comparator rejects injected bookkeeping faults (last key
dropped, last key counted twice, K rolled by one row), and a CPU emulation of the kernels' arithmetic (16-bit P, fp32
accumulation, 16-bit store) lands on the right side of the tolerance with and without each fault - which is what makes
tests/test_attention_structured_gpu.py meaningful."""
import pytest
import torch

import attn_patterns as ap

# every sequence length the GPU file uses; (B, H) = (2, 2) below the long-sequence kernel, (1, 1) from 4096 on
SIZES_BF16 = (1, 33, 64, 65, 129, 255, 256, 259, 288, 289, 300, 643, 4096, 4099, 4131)
SIZES_F16 = (77, 300, 643, 4131)
ALL_SIZES = tuple(sorted(set(SIZES_BF16 + SIZES_F16)))
DTYPES = (torch.bfloat16, torch.float16)


def shape_of(S):
    return (2, S, 2) if S < 4096 else (1, S, 1)


def build(kind, S, arg=None):
    B, S, H = shape_of(S)
    if kind == "census":
        return ap.census(B, S, H, *arg)
    return ap.selector(B, S, H, seed=1) if kind == "selector" else ap.peaked(B, S, H, seed=1)


def check(kind, got, p, ref=None):
    if kind == "census":
        return ap.check_census(got, p)
    return ap.check_selector(got, p) if kind == "selector" else ap.check_peaked(got, p, ref)


@pytest.mark.parametrize("S", ALL_SIZES)
def test_census_builder_claims(S):
    B, S, H = shape_of(S)
    for cmap in ap.CENSUS_MAPS:
        cls = ap.census_classes(B, S, H, cmap)
        for c in ap.CENSUS_SCORES:
            p = ap.census(B, S, H, c, cmap)                      # asserts 16-bit exactness and the class-count condition
            for b in range(B):
                for h in range(H):
                    s = ap.scores_of(p, b, h)
                    assert float(s.min()) == float(s.max()) == float(c)
                    assert torch.equal(p.counts[b, h], torch.bincount(cls[b, :, h], minlength=64))
            nz = p.counts[p.counts > 0]
            assert int(nz.min()) <= ap.CENSUS_MAX_MIN_COUNT and S <= 4600
            assert p.qk_bound <= ap.PEAKED_BOUND                 # inside the a-priori bound: the bounded-score loop
        if B > 1 and S > 1:                                      # heads and batches carry different class maps
            assert not torch.equal(cls[0, :, 0], cls[0, :, 1]) and not torch.equal(cls[0, :, 0], cls[1, :, 0])
    if S >= 64:
        a = ap.census(B, S, H, 0, "A").counts
        assert int(a.min()) >= 1                                  # map A: every class in every (batch, head)
        bmap = ap.census_classes(B, S, H, "B")[0, :, 0]
        assert bool(((bmap[1:] - bmap[:-1]) % 64 <= 1).all())     # map B: contiguous blocks


@pytest.mark.parametrize("S", ALL_SIZES)
def test_selector_builder_claims(S):
    B, S, H = shape_of(S)
    p = ap.selector(B, S, H, seed=1)                             # asserts 16-bit exactness and margin >= 64
    assert p.margin >= ap.SELECTOR_MIN_MARGIN
    assert p.qk_bound > ap.PEAKED_BOUND                          # outside the a-priori bound: never the bounded-score loop
    assert bool((p.v != 0).all()) and float(p.v.abs().max()) <= 127 / 32
    for b in range(B):
        for h in range(H):
            s = ap.scores_of(p, b, h)
            assert torch.equal(s.argmax(dim=1), p.perm[b, h])     # row i selects key perm(i) ...
            assert torch.equal(p.perm[b, h].sort().values, torch.arange(S))      # ... and every key is selected once
            top = s.max(dim=1).values
            assert float(top.min()) == float(top.max()) == p.match
            if S > 1:
                s2 = s.clone()
                s2[torch.arange(S), p.perm[b, h]] = float("-inf")
                assert float(s2.max()) == p.match - p.margin
    if B > 1 and S > 2:
        assert not torch.equal(p.perm[0, 0], p.perm[0, 1]) and not torch.equal(p.perm[0, 0], p.perm[1, 0])
        assert not torch.equal(p.v[0, :, 0], p.v[0, :, 1]) and not torch.equal(p.v[0, :, 0], p.v[1, :, 0])


def test_selector_scores_quoted_in_the_gpu_file():
    got = {S: (ap.selector(1, S, 1).match, ap.selector(1, S, 1).margin) for S in (33, 259, 643, 4131)}
    assert got == {33: (480.0, 160.0), 259: (504.0, 112.0), 643: (480.0, 96.0), 4131: (416.0, 64.0)}
    with pytest.raises(AssertionError):
        ap.selector(1, 65537, 1)                                  # 17 bits: 3 copies, margin 48


@pytest.mark.parametrize("S", sorted(ap.PEAKED_SCALES))
def test_peaked_builder_claims(S):
    B, S, H = shape_of(S)
    p = ap.peaked(B, S, H, seed=1)
    assert (p.match, p.margin) == {643: (60.0, 12.0), 4131: (78.0, 12.0)}[S]
    assert p.qk_bound == p.match <= ap.PEAKED_BOUND
    for b in range(B):
        for h in range(H):
            qn = p.q[b, :, h].double().norm(dim=-1).max()
            kn = p.k[b, :, h].double().norm(dim=-1).max()
            assert abs(float(qn * kn) - p.qk_bound) < 1e-9
            s = ap.scores_of(p, b, h)
            assert torch.equal(s.argmax(dim=1), p.perm[b, h]) and float(s.max()) == p.match


CASES = [("census", S, (c, m)) for S in ALL_SIZES for c in ap.CENSUS_SCORES for m in ap.CENSUS_MAPS] + \
        [("selector", S, None) for S in ALL_SIZES] + [("peaked", S, None) for S in sorted(ap.PEAKED_SCALES)]


def _id(case):
    kind, S, arg = case
    return f"{kind}-{S}" + (f"-c{arg[0]}-{arg[1]}" if arg else "")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_reference_and_emulation_pass_and_injected_faults_fail(case):
    """For the fp64 softmax rounded to the output type (the best a kernel can do) and for the CPU emulation of the
    kernels' arithmetic: the comparator accepts the clean result and rejects every fault the pattern is meant to catch."""
    kind, S, arg = case
    p = build(kind, S, arg)
    ref = ap.softmax_ref(p.q, p.k, p.v)
    if kind == "census":
        assert torch.equal(ref, ap.census_expected(p)) or float((ref - ap.census_expected(p)).abs().max()) < 1e-15
    if kind == "selector":
        assert torch.equal(ref, ap.selector_expected(p, torch.float64)), "fp64 softmax differs from V[perm]"
    for fault in (None,) + (ap.CATCHES[kind] if S >= 2 else ()):       # one key: nothing to drop, and its copy changes nothing
        k, v = ap.inject(p, fault)
        ref_f = ap.softmax_ref(p.q, k, v) if fault else ref
        for dtype in DTYPES:
            for name, got in (("reference", ref_f.to(dtype)), ("emulation", ap.emulate(p.q, k, v, dtype))):
                ok, worst, msg = check(kind, got, p, ref)
                if fault is None:
                    assert ok, (name, dtype, msg)
                else:
                    assert not ok, (name, dtype, fault, "an injected fault passed the comparator", msg)
                    assert worst >= 2.0, (name, dtype, fault, worst)      # no fault sits near the tolerance
                if kind != "selector":
                    print(f"{_id(case)} {name} {dtype} {fault or 'clean'}: error = {worst:.3f} x tolerance")
