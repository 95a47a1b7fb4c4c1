"""The full e4m3 stack on token-sharded layouts at the model level: enable_qk8_attention(pv8=True, fused_producer=True, cross=True,
smooth_v=True, smooth_v_cross=True, sharded="all") on the dim-3072 model of tests/test_token_shard_invariance.py with emulated ranks.  The
kernels and the switch: tests/test_attention_shard8s.py.  No multi-GPU hardware run exists: the ranks are emulated on one GPU."""
import pytest
import torch

import test_attention_shard8 as shard8
import test_token_shard_invariance as tsi
from fairygen_amd import hip as _hip
from test_token_shard_invariance import medium  # noqa: F401  (the module fixture)

gpu = pytest.mark.gpu
FULL = dict(pv8=True, fused_producer=True, cross=True, smooth_v=True, smooth_v_cross=True)
N = 1950


class CutShard(shard8.RecordShard):
    """A RecordShard whose rows are dealt by given cuts instead of the ceil split, so that a rank can be left without rows at N = 1 950
    (the ceil split does that only where N is small against the world).  The mailbox concatenates what the ranks deposit."""

    def __init__(self, box, rank, attn_mode, cuts):
        super().__init__(box, rank, attn_mode)
        self.cuts = cuts

    def local_range(self, n, rank=None):
        rank = self.rank if rank is None else rank
        assert n == self.cuts[-1]
        return self.cuts[rank], self.cuts[rank + 1]


def run_ranks(dit, world, attn_mode, cuts=None, **call):
    from fairygen_amd.wan_video import model_fn_wan_video_steps, run_interleaved
    box = tsi.Mailbox(world)
    shards = [shard8.RecordShard(box, r, attn_mode) if cuts is None else CutShard(box, r, attn_mode, cuts) for r in range(world)]
    results = run_interleaved([model_fn_wan_video_steps(dit, sequence_shard=s, gather_output=False, **call) for s in shards])
    for s, (out, _) in zip(shards, results):
        lo, hi = s.local_range(N)
        assert out.shape[:2] == (1, hi - lo), (s.rank, out.shape, (lo, hi))
    return dit.unpatchify(torch.cat([out for out, _ in results], dim=1), results[0][1]), box


_whole = {}
CASES = [("allgather", 3, None), ("ulysses", 2, None), ("allgather", 3, (0, 975, 975, N))]


@gpu
@pytest.mark.parametrize("attn_mode,world,cuts", CASES, ids=["allgather-P3", "ulysses-P2", "allgather-P3-empty-rank"])
def test_emulated_ranks_equal_unsharded_forward(medium, attn_mode, world, cuts):  # noqa: F811
    """P emulated ranks against the unsharded forward WITH THE SAME SWITCHES, under the criterion test_attention_shard8.py applies to the
    pv8 mode: the operand bytes are identical, only the k-split and split-KV grouping can differ, the bound is
    tests/test_token_shard_invariance.py's 2 err_ref + 1e-2 (err_ref = max|oracle bf16 - oracle fp32|).  allgather P = 3: 650 rows each;
    the third case deals (975, 0, 975) rows: the middle rank launches nothing, sends neutral records and no K / V rows, and contributes
    no output rows.  Every exchange of every block ran; every rank with rows ran the smoothed e4m3 self-attention and the smoothed e4m3
    cross-attention kernel once per block, and no bf16 attention kernel ran."""
    from fairygen_amd.wan_video import model_fn_wan_video
    dit = medium.dit
    medium.setting(False, True)
    names, real = [], _hip._call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    try:
        with torch.no_grad():
            if "full" not in _whole:
                dit.enable_qk8_attention(**FULL)
                _whole["full"] = model_fn_wan_video(dit, **medium.call).float().cpu()
            dit.enable_qk8_attention(sharded="all", **FULL)
            with pytest.MonkeyPatch.context() as patch:
                patch.setattr(_hip, "_call", call)
                out, box = run_ranks(dit, world, attn_mode, cuts, **medium.call)
    finally:
        dit.enable_qk8_attention(False)
    out, want = out.float().cpu(), _whole["full"]
    working = world if cuts is None else sum(hi > lo for lo, hi in zip(cuts, cuts[1:]))
    assert box.completed == 2 * len(dit.blocks) and not box.slots, "not every exchange of every block ran"
    assert names.count("fg_attn_fwd_pv8s_bf16") == working * len(dit.blocks), "self-attention did not take the smoothed e4m3 kernel once per rank and block"
    assert names.count("fg_attn_fwd_cross8s_bf16") == working * len(dit.blocks), "cross-attention did not take the smoothed e4m3 kernel"
    assert not any(n in names for n in ("fg_attn_fwd_bf16", "fg_attn_fwd_pv8_bf16", "fg_attn_fwd_qk8_bf16", "fg_attn_fwd_cross8_bf16"))
    if attn_mode == "allgather":
        assert names.count("fg_attn_shard8s_stats") == names.count("fg_attn_shard8s_quant") == working * len(dit.blocks)
        assert "fg_attn_shard8_stats" not in names and "fg_attn_shard8_quant" not in names
    bound = 2 * medium.err_ref + 1e-2
    diff = (out - want).abs().max().item()
    print(f"emulated {attn_mode} P={world}{' (one empty rank)' if cuts else ''}, full e4m3 stack: max|emulated - unsharded| = {diff:.5f}, "
          f"err_ref = {medium.err_ref:.5f}, bound = {bound:.5f}, max|unsharded| = {want.abs().max().item():.3f}")
    assert torch.isfinite(out).all() and out.shape == want.shape
    assert diff <= bound, f"emulated ranks differ from the unsharded forward of the mode by {diff} (bound {bound})"
