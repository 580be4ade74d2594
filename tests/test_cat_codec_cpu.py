"""Host-side pieces of gauspcc_amd.cat_codec (no GPU): the stage table of CAT-3DGS's channel-wise context chain, the pipeline schedule of
gsac_decode_normal_chain restated in a few lines, and the chain's class and switch (the slice geometry: tests/test_anchor_codec_cpu.py)."""
import types

import pytest
import torch

from gauspcc_amd import cat_codec

F, K = 50, 10
CONFIGS = [([12, 12, 13, 13], False, False), ([12, 12, 13, 13], True, True), ([5, 10, 15, 20], False, True), ([25, 25], True, False), ([50], False, False),
           ([50], True, True)]


def _model(groups, on_s, on_o, n_offsets=K):
    m = types.SimpleNamespace(feat_dim=F, n_offsets=n_offsets, chcm_slices_list=list(groups), num_feat_slices=len(groups),
                              mlp_chcm_list=[f"mlp{i}" for i in range(len(groups) - 1)], chcm_for_scaling=on_s, chcm_for_offsets=on_o)
    if on_s:
        m.mlp_chcm_scaling = "mlp_s"
    if on_o:
        m.mlp_chcm_offsets = "mlp_o"
    return m


@pytest.mark.parametrize("groups,on_s,on_o", CONFIGS)
@pytest.mark.parametrize("n_offsets", [5, 10])
def test_stage_table(groups, on_s, on_o, n_offsets):
    st = cat_codec.stage_table(_model(groups, on_s, on_o, n_offsets))
    G, k3 = len(groups), 3 * n_offsets
    assert [s["name"] for s in st] == [f"feat{i}" for i in range(G)] + ["scaling", "offsets"]
    assert [s["stem"] for s in st] == [s["name"] for s in st]
    # the context row (CAT-3DGS/scene/gaussian_model.py:1227-1228): scales, means, mean_scaling, scale_scaling, mean_offsets, scale_offsets, 3 adjustments
    width = 2 * F + 12 + 2 * k3 + 3
    c0 = 0
    for i, (s, ch) in enumerate(zip(st, groups)):
        assert (s["ch"], s["scale_col"], s["mean_col"], s["out_col"], s["feat_col"]) == (ch, c0, F + c0, c0, c0)
        assert s["dep_ch"] == (c0 if i else 0) and s["lag"] == i and s["attr"] == "feat" and s["q_col"] == width - 3
        assert s["mlp"] == (f"mlp{i - 1}" if i else None)
        c0 += ch
    sc, of = st[G], st[G + 1]
    assert (sc["ch"], sc["mean_col"], sc["scale_col"], sc["q_col"], sc["feat_col"]) == (6, 2 * F, 2 * F + 6, width - 2, -1)
    assert (of["ch"], of["mean_col"], of["scale_col"], of["q_col"], of["feat_col"]) == (k3, 2 * F + 12, 2 * F + 12 + k3, width - 1, -1)
    assert (sc["dep_ch"], sc["lag"], sc["mlp"]) == ((F, G, "mlp_s") if on_s else (0, 0, None))
    assert (of["dep_ch"], of["lag"], of["mlp"]) == ((F, G, "mlp_o") if on_o else (0, 0, None))
    # every column a stage reads lies inside the row, and the mean / scale ranges of all stages tile columns [0, width - 3) exactly once
    cols = sorted(c for s in st for base in (s["mean_col"], s["scale_col"]) for c in range(base, base + s["ch"]))
    assert cols == list(range(width - 3))
    assert len(st) == G + 2 <= cat_codec.CHAIN_MAX_STAGES


@pytest.mark.parametrize("groups,on_s,on_o", CONFIGS)
@pytest.mark.parametrize("n_anchors", [1, 37, 499, 500])
@pytest.mark.parametrize("block", [1, 7, 8, 16, 64])
def test_schedule_reads_only_what_earlier_steps_wrote(groups, on_s, on_o, n_anchors, block):
    """The kernel's schedule in a few lines: in step t stage k decodes block t - lag_k.  Every block of a channel a stage's MLP reads was decoded in an
    EARLIER step (the step barrier separates them), every stage decodes every block exactly once and in order, and the loop has nblocks + max_lag steps."""
    st = cat_codec.stage_table(_model(groups, on_s, on_o))
    lags = [s["lag"] for s in st]
    nblocks = -(-n_anchors // block)
    written = {}                                            # (stage, block) -> step
    steps = 0
    t = 0
    while len(written) < len(st) * nblocks:
        for k, s in enumerate(st):
            b = t - s["lag"]
            if 0 <= b < nblocks:
                for j, p in enumerate(st):                  # the stages that decode a channel below dep_ch
                    if p["feat_col"] >= 0 and p["feat_col"] < s["dep_ch"]:
                        assert (j, b) in written and written[(j, b)] < t, (k, j, b, t)
                assert (k, b) not in written and (b == 0 or written[(k, b - 1)] == t - 1)
        for k, s in enumerate(st):                          # the step's writes land at its barrier
            b = t - s["lag"]
            if 0 <= b < nblocks:
                written[(k, b)] = t
        t += 1
        steps = t
    assert steps == nblocks + max(lags) == cat_codec.chain_steps(n_anchors, block, lags)
    sched = cat_codec.chain_schedule(n_anchors, block, lags)
    assert len(sched) == steps and all(len(row) == len(st) for row in sched)
    for (k, b), step in written.items():
        assert sched[step][k] == b
    assert sum(v is not None for row in sched for v in row) == len(st) * nblocks
    # the window of max_lag + 1 blocks: a slot is overwritten (by block b + W) only after the last step that reads block b
    W = max(lags) + 1
    for b in range(nblocks - W):
        last_read = b + max(lags)
        assert min(written[(k, b + W)] for k, s in enumerate(st) if s["feat_col"] >= 0) > last_read


def test_chain_class_and_switch(monkeypatch):
    lin = torch.nn.Linear
    mk = lambda din, dh, dout: torch.nn.Sequential(lin(din, dh), torch.nn.ReLU(True), lin(dh, dout))   # noqa: E731
    m = _model([25, 25], True, False)
    m.mlp_chcm_list = [mk(25, 100, 50)]
    m.mlp_chcm_scaling = mk(50, 100, 12)
    st = cat_codec.stage_table(m)
    assert cat_codec.chain_eligible(st)
    monkeypatch.delenv("GAUSPCC_DEV", raising=False)
    monkeypatch.setenv("GAUSPCC_CAT_CHAIN", "0")            # ignored without GAUSPCC_DEV=1
    assert cat_codec._use_chain(None, st, 10) is True and cat_codec._use_chain(False, st, 10) is False and cat_codec._use_chain(True, st, 10) is True
    # chain=None: the kernel below CHAIN_AUTO_MAX_SLICES slices, the staged path from there (and for nothing to decode)
    assert cat_codec._use_chain(None, st, 500 * (cat_codec.CHAIN_AUTO_MAX_SLICES - 1)) is True
    assert cat_codec._use_chain(None, st, 500 * (cat_codec.CHAIN_AUTO_MAX_SLICES - 1) + 1) is False and cat_codec._use_chain(None, st, 0) is False
    assert cat_codec._use_chain(True, st, 1_000_000) is True
    monkeypatch.setenv("GAUSPCC_DEV", "1")
    assert cat_codec._use_chain(None, st, 10) is False and cat_codec._use_chain(True, st, 10) is False
    monkeypatch.setenv("GAUSPCC_CAT_CHAIN", "1")
    assert cat_codec._use_chain(False, st, 10) is True
    monkeypatch.delenv("GAUSPCC_DEV")
    # outside the kernel's class: 129 hidden units, a context MLP of another shape, more than 8 stages
    m.mlp_chcm_scaling = mk(50, 129, 12)
    assert not cat_codec.chain_eligible(cat_codec.stage_table(m))
    m.mlp_chcm_scaling = torch.nn.Sequential(lin(50, 12))
    st = cat_codec.stage_table(m)
    assert not cat_codec.chain_eligible(st) and cat_codec._use_chain(None, st, 10) is False
    with pytest.raises(ValueError):
        cat_codec._use_chain(True, st, 10)
    m7 = _model([8, 7, 7, 7, 7, 7, 7], False, False)
    m7.mlp_chcm_list = [mk(8 + 7 * i, 100, 14) for i in range(6)]
    assert not cat_codec.chain_eligible(cat_codec.stage_table(m7))
