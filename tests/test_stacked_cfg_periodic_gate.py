"""The stacked CFG forward with its two-row gated stores in ONE launch per Linear (WanModel.enable_stacked_cfg(periodic_gate=True),
ModelConfig(stacked_cfg_periodic_gate=True)): self_attn.o and ffn.2 of a TI2V block run fg_gemm_epilogue_bf16_sp / fg_gemm_fp8_bf16_sp
(include/fairygen_hip_gategemm.h) on the 2 N rows of the pair with rows_per_element = N, instead of the _s entry point once per element.

The model, inputs and oracle references are those of tests/test_stacked_cfg_forward.py (imported; the references are computed once per
process and shared), at N = 1 200: the 2 400 stacked rows are 120 tiles at 3072 columns, which own_gemm_ok takes as they are — the 1 200
rows of one element (60 tiles) are under its floor, so WITHOUT the opt-in these stores run on library GEMMs and the batched row kernels.

EXACT: with the two seams of wan_video_dit.py replaced by "the same launch in mode 0 (bias only) + torch's bf16 gate add", the forward is
bit-equal (mode 0 and mode 2 of a shape share their plan; tests/test_gemm_periodic_gate.py holds the kernels).  ORACLE: nothing wrapped,
each element under the bound test_stacked_cfg_forward.test_stacked_vs_oracle uses: err <= 2 err_ref + 1e-2 and cos > 0.9995 against the
fp32 oracle, err_ref the bf16 oracle's own error.  Once more in the fp8 Linear mode with unfused adapters on the HIP backend, where the
oracle is Fp8Blocks with lora_forward's sum behind every adapted Linear.  COUNT: the new entry points are called 3 times per forward of
2 blocks with the opt-in (block 0's self-attention half is shared and runs on one element) and never without it.
"""
import pytest
import torch

from fairygen_amd import synthetic
from oracle import wan_dit
from test_stacked_cfg_forward import MEDIUM, _medium_inputs, _model, _oracle, cos
from test_stacked_cfg_hot_lora import _adapters, _attach

gpu = pytest.mark.gpu
N = 1200
NEW = ("fg_gemm_epilogue_bf16_sp", "fg_gemm_fp8_bf16_sp")


# ------------------------------------------------------------------------------------------------------------------ CPU: the switch
def test_opt_in_is_off_by_default_and_stated_with_every_call():
    from fairygen_amd import ModelConfig
    from fairygen_amd.wan_video_dit import WanModel
    m = WanModel(**synthetic.TINY_DIT_KWARGS)
    assert m.stacked_cfg is False and m.stacked_cfg_periodic_gate is False
    assert m.enable_stacked_cfg() is m and m.stacked_cfg is True and m.stacked_cfg_periodic_gate is False
    assert m.enable_stacked_cfg(periodic_gate=True) is m and m.stacked_cfg_periodic_gate is True
    assert m.stacked_cfg_fp8 is False and m.stacked_cfg_hot_lora is False
    assert m.enable_stacked_cfg(True).stacked_cfg_periodic_gate is False      # cleared by a call that does not restate it
    m.enable_stacked_cfg(fp8_linear=True, hot_lora=True, periodic_gate=True)      # composes with the other two
    assert m.stacked_cfg_fp8 and m.stacked_cfg_hot_lora and m.stacked_cfg_periodic_gate
    assert m.enable_stacked_cfg(False, periodic_gate=True).stacked_cfg_periodic_gate is False      # nothing to opt into with the switch off
    cfg = ModelConfig(path="x")
    assert cfg.stacked_cfg_periodic_gate is False and cfg.vram_config()["stacked_cfg_periodic_gate"] is False
    assert ModelConfig(path="x", stacked_cfg=True, stacked_cfg_periodic_gate=True).vram_config()["stacked_cfg_periodic_gate"] is True
    with pytest.raises(ValueError, match="needs stacked_cfg=True"):
        ModelConfig(path="x", stacked_cfg_periodic_gate=True).check_input()


def test_refusals_stand_with_the_opt_in():
    """Host tensors: token shards, windows, a context batch other than 2 and the fp8 mode without its own opt-in raise as without it."""
    import types
    from fairygen_amd.wan_video import model_fn_wan_video
    from test_stacked_cfg_forward import _tiny_inputs
    m, _ = _model(synthetic.TINY_DIT_KWARGS, 1234, "cpu")
    m.enable_stacked_cfg(periodic_gate=True)
    lat, ctx_p, ctx_n, _, ts = _tiny_inputs()
    both = torch.cat([ctx_p, ctx_n], 0)
    call = lambda **kw: model_fn_wan_video(m, **{**dict(latents=lat, timestep=ts, context=both, fuse_vae_embedding_in_latents=True), **kw})      # noqa: E731
    with pytest.raises(NotImplementedError, match="context batch of 2, not 3"):
        call(context=torch.cat([both, ctx_p], 0))
    with pytest.raises(NotImplementedError, match="sliding windows"):
        call(sliding_window_size=2, sliding_window_stride=1)
    with pytest.raises(NotImplementedError, match="active token shard"):
        call(sequence_shard=types.SimpleNamespace(active=True))
    m.enable_fp8_linear()
    with pytest.raises(NotImplementedError, match="enable_fp8_linear"):
        call()


# ------------------------------------------------------------------------------------------------------------------ GPU
def _merged(m, lat, ts, both, periodic, hot=False):
    from fairygen_amd.wan_video import model_fn_wan_video
    m.enable_stacked_cfg(True, fp8_linear=m.fp8_dtype is not None, hot_lora=hot, periodic_gate=periodic)
    try:
        with torch.no_grad():
            return model_fn_wan_video(m, latents=lat, timestep=ts, context=both, fuse_vae_embedding_in_latents=True)
    finally:
        m.enable_stacked_cfg(False)


def _count_new_entry_points(monkeypatch):
    """Every call of the library's two new entry points, by name."""
    from fairygen_amd import hip
    seen, real = [], hip._call

    def call(name, *args):
        if name in NEW:
            seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(hip, "_call", call)
    return seen


def _gate_add(x, y, mod, gate_idx):
    """x (B, rows, N) += gate[class(row inside the element)] * y in torch's bf16 ops: one rounding per op."""
    cls = (torch.arange(x.shape[1], device=x.device) >= mod.first_rows).long()
    x.copy_(x + mod.table[cls, gate_idx] * y.view_as(x))
    return x


def _mode0_seams(monkeypatch):
    """The two periodic seams as the SAME launch (rows, scratch, scheduler block) in mode 0, then the gate add above."""
    from fairygen_amd import hip, wan_video_dit as D
    used = []

    def bf16(x, a, weight, bias, mod, gate_idx, rows_per_element, **state):
        used.append(("bf16", a.shape[0], rows_per_element, mod.mod_rows))
        return _gate_add(x, hip.gemm_epilogue(a, weight, bias, **state), mod, gate_idx)

    def fp8(x, xq, scale_a, w8, bias, mod, gate_idx, rows_per_element, **state):
        used.append(("fp8", xq.shape[0] // rows_per_element, rows_per_element, mod.mod_rows))
        return _gate_add(x, hip.gemm_fp8(xq, scale_a, w8, bias, **state), mod, gate_idx)
    monkeypatch.setattr(D, "gemm_residual_periodic", bf16)
    monkeypatch.setattr(D, "gemm_fp8_residual_periodic", fp8)
    return used


def _check_oracle(got, refs, what):
    for e, (ref16, ref32) in enumerate(refs):
        err_ref = (ref16.float() - ref32).abs().max().item()
        err = (got[e:e + 1].float().cpu() - ref32).abs().max().item()
        print(f"{what}: element {e}: err {err:.5f} err_ref {err_ref:.5f} cos {cos(got[e:e + 1], ref32):.6f}")
        assert err <= 2 * err_ref + 1e-2, (e, err, err_ref)
        assert cos(got[e:e + 1], ref32) > 0.9995, e


@pytest.fixture(scope="module")
def medium():
    return _model(MEDIUM, 99, "cuda")


@gpu
def test_periodic_forward_bf16(monkeypatch, medium):
    """bf16 Linears, TI2V (first_rows = 400 inside the 1 200 rows of an element).  Unwrapped: 3 calls of fg_gemm_epilogue_bf16_sp, each
    element under the oracle bound.  With the mode-0 seams: no call of it, and the same bits.  Without the opt-in: no call of it."""
    from fairygen_amd import wan_video_dit as D
    m, sd = medium
    assert D.own_gemm_ok(2 * N, 3072, 3072) and D.own_gemm_ok(2 * N, 3072, 1024) and not D.own_gemm_ok(N, 3072, 3072)
    lat, both, ts = _medium_inputs(N)
    lat, both = lat.cuda(), both.cuda()
    seen = _count_new_entry_points(monkeypatch)
    off = _merged(m, lat, ts, both, False)
    assert seen == [], "without the opt-in the new entry points are never called"
    got = _merged(m, lat, ts, both, True)
    assert seen == [NEW[0]] * 3, seen
    assert not torch.equal(got[0], got[1])
    _check_oracle(got, _oracle(sd, N, True), "periodic gate, bf16")
    _check_oracle(off, _oracle(sd, N, True), "no opt-in, bf16")
    del seen[:]
    used = _mode0_seams(monkeypatch)
    want = _merged(m, lat, ts, both, True)
    assert seen == [] and used == [("bf16", 2, N, 2)] * 3, (seen, used)
    assert torch.equal(got, want)


_REFS8 = {}


def _oracle_fp8_adapters(monkeypatch, sd, adapters):
    """(ref_bf16, ref_f32) per element of the fp8 Linear mode with lora_forward's sum behind every adapted Linear, computed once."""
    if not _REFS8:
        real = wan_dit.linear

        def linear(sd_, prefix, x):      # oracle.wan_dit.linear, then the adapters on the same input (core/vram/layers.py:417-436)
            out = real(sd_, prefix, x)
            for a, b in adapters.get(prefix, ()):
                out = out + x @ a.to(x.dtype).T @ b.to(x.dtype).T
            return out
        monkeypatch.setattr(wan_dit, "linear", linear)
        lat, both, ts = _medium_inputs(N)
        sd32 = {k: v.float() for k, v in sd.items()}
        _REFS8["refs"] = [(wan_dit.model_fn(wan_dit.Fp8Blocks(sd), MEDIUM, lat, ts, both[e:e + 1], True),
                           wan_dit.model_fn(wan_dit.Fp8Blocks(sd32), MEDIUM, lat.float(), ts.float(), both[e:e + 1].float(), True)) for e in range(2)]
        monkeypatch.setattr(wan_dit, "linear", real)
    return _REFS8["refs"]


@gpu
def test_periodic_forward_fp8_with_hip_adapters(monkeypatch):
    """The fp8 Linear mode with unfused adapters on the HIP backend (hot_lora=True): the gated stores are fg_gemm_fp8_bf16_sp on the 2 N
    quantised rows, the adapter launch behind each stays the one batched launch.  The same three checks."""
    from fairygen_amd import hip
    m, sd = _model(MEDIUM, 99, "cuda")
    m.enable_fp8_linear()
    adapters = _adapters(MEDIUM)
    _attach(m, adapters)
    lat, both, ts = _medium_inputs(N)
    lat, both = lat.cuda(), both.cuda()
    seen = _count_new_entry_points(monkeypatch)
    lora = []
    real_lora = hip.lora_apply
    monkeypatch.setattr(hip, "lora_apply", lambda *a, **kw: (lora.append((kw.get("mode", "add"), kw.get("batch"))), real_lora(*a, **kw))[1])
    _merged(m, lat, ts, both, False, hot=True)
    assert seen == [], "without the opt-in the new entry points are never called"
    lora_off = list(lora)
    del lora[:]
    got = _merged(m, lat, ts, both, True, hot=True)
    assert seen == [NEW[1]] * 3, seen
    assert lora == lora_off and lora.count(("gate", 2)) == 3      # the adapter launches are what they were: one batched launch per store
    assert not torch.equal(got[0], got[1])
    del seen[:]
    used = _mode0_seams(monkeypatch)
    want = _merged(m, lat, ts, both, True, hot=True)
    assert seen == [] and used == [("fp8", 2, N, 2)] * 3, (seen, used)
    assert torch.equal(got, want)
    _check_oracle(got, _oracle_fp8_adapters(monkeypatch, sd, adapters), "periodic gate, fp8 + hip adapters")
