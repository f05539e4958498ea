"""pi3_attention on inputs whose exact answer is known (tests/attn_patterns.py), through every dispatch path of the
product library and every value of the knobs that choose a softmax loop.

The accuracy tests of the attention kernels compare Gaussian q/k/v with an fp32 softmax under a gate of 8e-3, at the
default knobs.  A mishandled key shows there only as far as some row happens to weight it by a few percent, and there
is no exact answer to hold a kernel to.  Here one key dropped, counted twice or read from the wrong row or ring slot is
an O(1) error with a derived tolerance, on every loop that a knob can select:
  census    uniform scores (0, +48, -48), one-hot class V: out = n / S within the rounding of the 16-bit store
            (2^-8 relative for bf16, 2^-11 for half), exactly 0 for empty classes;
  selector  one-hot softmax: out[i] == V[perm(i)] bit for bit; match scores 416 ... 512 overflow the loop without a
            running maximum on purpose - the default form must reject and the follow-up launch deliver, the a-priori
            form must choose the online-max loop;
  peaked    the selector inside the bounded-score range (|q| max|k| = 60 / 78 <= 90) against the fp64 softmax, within
            2^-7 max|V|: the only O(1)-sensitive input the bounded-score loop can host.
The selector's margin assertion (>= 64) holds for every S <= 65 536, so no size below is left out of it.

Dispatch (attn.hip, attn64.hip): S < 256 the 32-row kernel (nt = 1 ... 4 key tiles and each `rem` branch that the
product reaches); 256 <= S < 4096 the four-wave 64-row kernel (259: last tile of 3 keys, `half_last`, the second
workgroup's waves own 1, 0, 0, 0 query blocks; 288 / 289: last tile of 32 / 33 keys, the two sides of the `half_last`
threshold; 300: last tile of 44 keys; 643: the frame size, the third workgroup owns 2, 2, 1, 0 blocks); S >= 4096 the
eight-wave kernels (4096: no tail; 4099, 4131: 3 and 35 tail keys).  IEEE half (MoGe) takes the 64-row kernel at every
length and always the online-max loop.  Census map A puts every class in every tile and so cannot see a tile counted in
place of another; map B (contiguous blocks) and the selector can.

Every output is prefilled with NaN and followed by three sentinel rows; q/k/v, perm and the class shifts differ per
(batch, head), so a read across a batch or head seam shows.  Each case prints its worst error in units of the tolerance."""
import pytest
import torch

import attn_patterns as ap

pytestmark = pytest.mark.gpu

ATTN_ASM_DEFAULT = 2        # knob attn_asm: 0 compiler-scheduled kernel, 2 hand-placed loop (attn_fwd64b_kernel)
ATTN_NOMAX_DEFAULT = 2      # knob attn_nomax: 0 online-max loop, 1 a-priori bound on |q| max|k|, 2 optimistic loop + redo
SENTINEL = 77.0
H = 2

# (attn_asm, attn_nomax, k2max supplied); knob 1 always with k2max (it reads it), knob 2 with and without, knob 0 ignores it
CFG_32ROW = [(ATTN_ASM_DEFAULT, ATTN_NOMAX_DEFAULT, False)]           # the 32-row kernel has no knobs
CFG_FOUR = [(ATTN_ASM_DEFAULT, 0, False), (ATTN_ASM_DEFAULT, 1, True), (ATTN_ASM_DEFAULT, 2, True), (ATTN_ASM_DEFAULT, 2, False)]
CFG_EIGHT = [(2, 2, True), (2, 2, False), (0, 2, True), (0, 2, False), (0, 1, True), (0, 0, False)]
SHAPES = [(2, S, CFG_32ROW) for S in (1, 33, 64, 65, 129, 255)] + [(2, S, CFG_FOUR) for S in (256, 259, 288, 289, 300, 643)] + \
         [(1, S, CFG_EIGHT) for S in (4096, 4099, 4131)]
BF16_CASES = [(B, S, cfg) for B, S, cfgs in SHAPES for cfg in cfgs]
F16_SHAPES = [(2, 77), (2, 300), (2, 643), (1, 4131)]
CENSUS = [(c, m) for c in ap.CENSUS_SCORES for m in ap.CENSUS_MAPS]


def _cfg_id(cfg):
    return f"asm{cfg[0]}-nomax{cfg[1]}-{'k2max' if cfg[2] else 'nok2max'}"


def _case_id(case):
    return f"B{case[0]}-S{case[1]}-{_cfg_id(case[2])}"


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pi3_slam_amd import lib
    lib.load(require_gpu=True)
    return torch.device("cuda:0")


_cache = {}


def pattern(dev, kind, B, S, arg=None):
    """(Pattern, {dtype: packed qkv on the device}, k2max, fp64 reference for `peaked`): built once per module."""
    key = (kind, B, S, arg)
    if key not in _cache:
        if kind == "census":
            p = ap.census(B, S, H, *arg)
        else:
            p = ap.selector(B, S, H, seed=3) if kind == "selector" else ap.peaked(B, S, H, seed=3)
        qkv = {dt: p.qkv(dt).to(dev) for dt in (torch.bfloat16, torch.float16)}
        k = qkv[torch.bfloat16].float().view(B, S, 3, H, 64)[:, :, 1]
        k2max = (k * k).sum(-1).amax(dim=1).reshape(-1).contiguous()      # what the fused qkv epilogue hands over
        ref = ap.softmax_ref(p.q.to(dev), p.k.to(dev), p.v.to(dev)) if kind == "peaked" else None
        _cache[key] = (p, qkv, k2max, ref)
    return _cache[key]


def run(dev, p, qkv, k2max, cfg, expect_empty_path=None):
    """One launch under the knobs of cfg into a NaN-prefilled output with sentinel rows -> the [B * S, H * 64] result.
    expect_empty_path: 0 / 1 = no wave may have taken its result from the bounded-score / online-max loop (asserted
    for bf16 on the 64-row kernels, where the path counters exist)."""
    from pi3_slam_amd import lib, ops
    asm, nomax, with_k2 = cfg
    B, S = p.B, p.S
    out = torch.full((B * S + 3, H * 64), float("nan"), device=dev, dtype=qkv.dtype)
    out[B * S:] = SENTINEL
    counted = qkv.dtype == torch.bfloat16 and S >= 256
    counters = torch.zeros(2, 2, 32, device=dev, dtype=torch.int32)
    try:
        lib.set_knob("attn_asm", asm)
        lib.set_knob("attn_nomax", nomax)
        if counted:
            ops.attention_path_counters(counters)
        ops.attention(qkv, out, B, S, H, k2max=k2max.clone() if with_k2 else None)
        torch.cuda.synchronize()
    finally:
        lib.set_knob("attn_asm", ATTN_ASM_DEFAULT)
        lib.set_knob("attn_nomax", ATTN_NOMAX_DEFAULT)
        torch.cuda.synchronize()
        ops.attention_path_counters(None)
    assert bool((out[B * S:] == SENTINEL).all()), "rows behind the output were written"
    if counted:
        w = counters.sum(-1).cpu()                         # [eight-wave | four-wave] x [bounded-score | online-max]
        kind = 0 if S >= 4096 else 1
        assert int(w[1 - kind].sum()) == 0 and int(w[kind].sum()) > 0, ("wrong kernel family", w.tolist())
        if expect_empty_path is not None:
            assert int(w[kind, expect_empty_path]) == 0, (f"waves took path {expect_empty_path}", w.tolist())
    return out[:B * S]


def report(what, ok, worst, msg):
    print(f"{what}: worst = {worst:.3f} x tolerance" if worst == worst and worst != float("inf") else f"{what}: {msg}")
    assert ok, (what, msg)


@pytest.mark.parametrize("case", BF16_CASES, ids=_case_id)
@pytest.mark.parametrize("c,cmap", CENSUS)
def test_census_bf16(dev, case, c, cmap):
    B, S, cfg = case
    p, qkv, k2max, _ = pattern(dev, "census", B, S, (c, cmap))
    # the a-priori form with max |k|^2 supplied: |q| max|k| = 48 <= 90 for every wave, so none may run the online-max loop
    out = run(dev, p, qkv[torch.bfloat16], k2max, cfg, expect_empty_path=1 if (cfg[1] == 1 and cfg[2]) else None)
    report(f"census c={c} map {cmap} S={S} {_cfg_id(cfg)} bf16", *ap.check_census(out, p))


@pytest.mark.parametrize("case", BF16_CASES, ids=_case_id)
def test_selector_bf16(dev, case):
    B, S, cfg = case
    p, qkv, k2max, _ = pattern(dev, "selector", B, S)
    # scores of 416 ... 512: no wave's result may come from the loop without a running maximum
    out = run(dev, p, qkv[torch.bfloat16], k2max, cfg, expect_empty_path=0)
    ok, n, msg = ap.check_selector(out, p)
    assert ok, (S, _cfg_id(cfg), msg)


@pytest.mark.parametrize("case", [c for c in BF16_CASES if c[1] in ap.PEAKED_SCALES], ids=_case_id)
def test_peaked_bf16(dev, case):
    B, S, cfg = case
    p, qkv, k2max, ref = pattern(dev, "peaked", B, S)
    out = run(dev, p, qkv[torch.bfloat16], k2max, cfg, expect_empty_path=1 if (cfg[1] == 1 and cfg[2]) else None)
    report(f"peaked S={S} {_cfg_id(cfg)} bf16", *ap.check_peaked(out, p, ref))


@pytest.mark.parametrize("B,S", F16_SHAPES)
@pytest.mark.parametrize("c,cmap", CENSUS)
def test_census_ieee_half(dev, B, S, c, cmap):
    p, qkv, k2max, _ = pattern(dev, "census", B, S, (c, cmap))
    out = run(dev, p, qkv[torch.float16], k2max, (ATTN_ASM_DEFAULT, ATTN_NOMAX_DEFAULT, False))
    report(f"census c={c} map {cmap} S={S} half", *ap.check_census(out, p))


@pytest.mark.parametrize("B,S", F16_SHAPES)
def test_selector_ieee_half(dev, B, S):
    p, qkv, k2max, _ = pattern(dev, "selector", B, S)
    out = run(dev, p, qkv[torch.float16], k2max, (ATTN_ASM_DEFAULT, ATTN_NOMAX_DEFAULT, False))
    ok, n, msg = ap.check_selector(out, p)
    assert ok, (S, msg)


@pytest.mark.parametrize("B,S", [(2, 65), (2, 259), (1, 4099)])
def test_selector_strided_qkv_and_output(dev, B, S):
    """include/pi3slam_hip.h promises arbitrary token strides: q/k/v as a column slice of a wider buffer (base 16-byte
    aligned, token stride wider than the packed row) and the output as a column slice of a wider buffer, one case per
    kernel family.  Everything around both slices is NaN: a read outside the slice poisons the result, a write outside
    it is seen."""
    from pi3_slam_amd import ops
    p, qkv, _, _ = pattern(dev, "selector", B, S)
    W = 3 * H * 64
    big = torch.full((B * S, W + 40), float("nan"), device=dev, dtype=torch.bfloat16)
    big[:, 8:8 + W] = qkv[torch.bfloat16]
    obig = torch.full((B * S + 3, H * 64 + 24), float("nan"), device=dev, dtype=torch.bfloat16)
    view = obig[:, 8:8 + H * 64]
    assert big[:, 8:8 + W].data_ptr() % 16 == 0 and view.data_ptr() % 8 == 0
    ops.attention(big[:, 8:8 + W], view, B, S, H)
    torch.cuda.synchronize()
    ok, n, msg = ap.check_selector(view[:B * S].contiguous(), p)
    assert ok, (S, msg)
    assert bool(torch.isnan(obig[:, :8]).all()) and bool(torch.isnan(obig[:, 8 + H * 64:]).all()) and \
        bool(torch.isnan(obig[B * S:]).all()), "the kernel wrote outside the output slice"
