"""CPU: the host side of MWER training (src/mwer.py) and the float64 reference it is pinned against
(tests/mwer_reference.py): the closed-form derivative, the options block, the n-best packing, the word mapping and the
condition of the end-to-end GPU case.

Two kinds of test live here.  Those on the product (the options, the packing, the word mapping, the argument checks of
the new entry points - the only place the latter are asserted) fail without the feature.  The others
(test_closed_form_gradient_equals_autograd, test_seq_logp_reference_gradient_is_the_documented_formula and the three
cases of test_end_to_end_case_has_spread_weights) check the REFERENCE and the fixed inputs alone: they hold whatever the
product does, and exist so that the GPU tests compare against something that was itself checked."""
import importlib

import numpy as np
import pytest
import torch

import mwer_reference as MR
from conftest import PKG_NAME


def _mwer():
    return importlib.import_module(PKG_NAME + ".src.mwer")


# ---- the derivative ----------------------------------------------------------------------------------------------------
def test_closed_form_gradient_equals_autograd():
    g = torch.Generator().manual_seed(0)
    N, U = 5, 6
    s = (torch.randn((N, U), generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    err = torch.randint(0, 9, (N, U), generator=g).numpy()
    err[:, 4] = 3                                      # all-equal errors
    count = [5, 3, 1, 0, 5, 2]                         # mixed, 1 and 0 among them
    loss_u, _, p = MR.mwer_loss(s, err, count)
    loss_u.sum().backward()
    loss_u = loss_u.detach()
    want = s.grad
    got = MR.closed_form_g(s, err, count)
    assert float((got - want).abs().max()) <= 1e-15
    # count 1 and all-equal errors: loss 0 and g = 0; invalid slots: 0
    assert float(loss_u[2].abs()) == 0.0 and float(got[:, 2].abs().max()) == 0.0
    assert float(loss_u[4].abs()) <= 1e-15 and float(got[:, 4].abs().max()) <= 1e-15
    assert float(loss_u[3]) == 0.0 and float(got[:, 3].abs().max()) == 0.0
    assert float(got[3:, 1].abs().max()) == 0.0 and float(got[:3, 1].abs().max()) > 0.0
    assert float(p[:, 0].sum()) == pytest.approx(1.0, abs=1e-15)


def test_seq_logp_reference_gradient_is_the_documented_formula():
    g = torch.Generator().manual_seed(1)
    M, V = 7, 11
    x = (torch.randn((M, V), generator=g, dtype=torch.float64) * 4).requires_grad_(True)
    tgt = torch.tensor([3, -1, 0, 10, 5, 2, 7])
    seg = [1, 3, 3, 6]                                 # row 0 and row 6 in no segment, one empty segment
    tok, seq, lse = MR.seq_logp(x, tgt, seg)
    w = torch.tensor([0.5, -2.0, 3.0], dtype=torch.float64)
    (seq * w).sum().backward()
    roww = torch.tensor([0, 0.5, 0.5, 3.0, 3.0, 3.0, 0], dtype=torch.float64)
    want = torch.zeros_like(x)
    for m in range(M):
        if tgt[m] >= 0:
            want[m] = -roww[m] * torch.exp(x[m].detach() - lse[m].detach())
            want[m, tgt[m]] += roww[m]
    assert float((x.grad - want).abs().max()) <= 1e-14
    assert float(seq[1].detach()) == 0.0 and float(tok[1].detach()) == 0.0


def test_argument_checks_need_no_gpu():
    """NULL pointers, negative sizes, short strides and N > 32 are refused before any device call; zero-size calls are
    ASRK_OK without a launch"""
    import ctypes
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    L = importlib.import_module(PKG_NAME + "._lib").load()
    z, f = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    assert L.asrk_seq_logp_lse_f32(f, 4, f, z, 1, 4, 0, 0, f, z, z, z) == -1          # no lse
    assert L.asrk_seq_logp_lse_f32(f, 3, f, z, 1, 4, 0, 0, f, f, z, z) == -1          # ldx < V
    assert L.asrk_seq_logp_lse_f32(f, 4, f, f, 1, 4, 1, 0, f, f, z, z) == -1          # seg_off without seq_logp
    assert L.asrk_seq_logp_lse_f32(f, 4, f, z, 0, 4, 0, 0, f, f, z, z) == 0           # empty
    assert L.asrk_seq_logp_bwd_f32(z, 4, f, f, f, f, 1, 4, 1, f, 4, z) == -1
    assert L.asrk_seq_logp_bwd_f32(f, 4, f, f, f, f, 1, 4, 1, z, 4, z) == -1
    assert L.asrk_seq_logp_bwd_f32(f, 4, f, f, f, f, 1, 4, 1, f, 3, z) == -1          # lddx < V
    assert L.asrk_seq_logp_bwd_f32(f, 4, f, f, f, f, -1, 4, 1, f, 4, z) == -1
    assert L.asrk_seq_logp_bwd_f32(f, 8, f, f, f, f, 1, 4, 1, f, 4, z) == -1          # in place, another stride
    assert L.asrk_seq_logp_bwd_f32(f, 4, f, f, z, f, 1, 4, 1, f, 4, z) == -1          # R > 0 without seg_off
    assert L.asrk_seq_logp_bwd_f32(f, 4, f, f, f, f, 0, 4, 1, f, 4, z) == 0
    assert L.asrk_mwer_loss_f64(f, f, f, 33, 2, f, f, f, z) == -2                     # ASRK_ESHAPE
    assert L.asrk_mwer_loss_f64(z, f, f, 4, 2, f, f, f, z) == -1
    assert L.asrk_mwer_loss_f64(f, f, z, 4, 2, f, f, f, z) == -1
    assert L.asrk_mwer_loss_f64(f, f, f, -1, 2, f, f, f, z) == -1
    assert L.asrk_mwer_loss_f64(f, f, f, 4, 0, f, f, f, z) == 0


# ---- options -----------------------------------------------------------------------------------------------------------
BLOCK = dict(enable=True, nbest=4, beam_size=4, ce_weight=0.01, unit='word', ctc_weight=0.0, min_len_ratio=0.01,
             max_len_ratio=0.30, start_step=0)


def _cfg(model_ctc=0.5, **kw):
    block = dict(BLOCK)
    block.update(kw)
    return {'model': {'ctc_weight': model_ctc}, 'mwer': block}


def test_options_accept_the_documented_block():
    M = _mwer()
    o = M.MWEROptions.from_config(_cfg())
    assert (o.nbest, o.beam_size, o.ce_weight, o.unit, o.ctc_weight, o.start_step) == (4, 4, 0.01, 'word', 0.0, 0)
    assert (o.min_len_ratio, o.max_len_ratio) == (0.01, 0.30)
    assert 'MWER' in o.create_msg()
    assert M.MWEROptions.from_config({'model': {'ctc_weight': 0.5}}) is None
    assert M.MWEROptions.from_config(_cfg(enable=False)) is None
    assert M.MWEROptions.from_config(_cfg(nbest=2, beam_size=32, unit='token', ctc_weight=0.3)).beam_size == 32
    assert M.MWEROptions.from_config({'model': {'ctc_weight': 0.0}, 'mwer': {'enable': True}}).nbest == 4


@pytest.mark.parametrize("bad", [dict(nbest=1), dict(nbest=33, beam_size=33), dict(nbest=True), dict(nbest=4.0),
                                 dict(beam_size=3), dict(unit='char'), dict(unit=None), dict(ce_weight=-0.1),
                                 dict(ce_weight='x'), dict(start_step=-1), dict(enable='yes'), dict(ctc_weight=1.0),
                                 dict(max_len_ratio=0.0), dict(bogus=1)])
def test_options_refuse_bad_values(bad):
    with pytest.raises(ValueError, match='mwer'):
        _mwer().MWEROptions.from_config(_cfg(**bad))


def test_options_refuse_models_the_criterion_does_not_cover():
    M = _mwer()
    with pytest.raises(ValueError, match='attention decoder'):
        M.MWEROptions.from_config(_cfg(model_ctc=1.0))
    with pytest.raises(ValueError, match='CTC head'):
        M.MWEROptions.from_config(_cfg(model_ctc=0.0, ctc_weight=0.2))
    cfg = _cfg()
    cfg['emb'] = {'enable': True}
    with pytest.raises(ValueError, match='emb.enable'):
        M.MWEROptions.from_config(cfg)
    cfg['emb'] = {'enable': False}
    assert M.MWEROptions.from_config(cfg) is not None
    with pytest.raises(ValueError, match='mapping'):
        M.MWEROptions.from_config({'mwer': [1]})


# ---- packing ------------------------------------------------------------------------------------------------------------
def test_pack_nbest_layout():
    M = _mwer()
    lists = [[[5, 6, 1], [5, 6], [7], [8, 9, 4, 3], [2]],      # a trailing <eos>, then the same hypothesis again
             [[4]],                                             # a short list
             [],                                                # nothing came back
             [[], [3, 1, 1]]]                                   # the empty hypothesis, a doubled <eos>
    ids, lens, count, hyps = M.pack_nbest(lists, 3)
    U = 4
    assert ids.shape == (3 * U, 5) and ids.dtype == torch.int64 and lens.dtype == torch.int64
    assert count.dtype == torch.int32 and count.tolist() == [3, 1, 1, 2]
    assert hyps == [[[5, 6], [7], [8, 9, 4, 3]], [[4]], [[]], [[], [3]]]
    row = lambda n, u: ids[n * U + u].tolist()
    # n-major rows, <eos> appended, zero padding
    assert row(0, 0) == [5, 6, 1, 0, 0] and row(1, 0) == [7, 1, 0, 0, 0] and row(2, 0) == [8, 9, 4, 3, 1]
    assert lens.view(3, U)[:, 0].tolist() == [3, 2, 5]
    # fillers beyond count: the utterance's first hypothesis
    assert row(0, 1) == row(1, 1) == row(2, 1) == [4, 1, 0, 0, 0] and lens.view(3, U)[:, 1].tolist() == [2, 2, 2]
    # an empty list: the hypothesis [] = <eos> alone
    assert row(0, 2) == row(1, 2) == [1, 0, 0, 0, 0] and lens.view(3, U)[:, 2].tolist() == [1, 1, 1]
    assert row(0, 3) == [1, 0, 0, 0, 0] and row(1, 3) == [3, 1, 0, 0, 0] and row(2, 3) == row(0, 3)
    # the independent packer of the reference agrees where its inputs are clean
    clean = [[[5, 6], [7], [8, 9, 4, 3]], [[4]], [], [[], [3]]]
    i2, l2, c2, _ = MR.pack(clean, 3)
    assert torch.equal(i2, ids) and torch.equal(l2, lens) and c2 == count.tolist()


# ---- words ---------------------------------------------------------------------------------------------------------------
def test_word_mapping_ignores_the_segmentation():
    M = _mwer()
    a, b, c = [3, 4, 6], [5, 7, 8], [5, 9]          # hello world / hello world / hello there
    hyp_w, ref_w = M.word_ids(MR.Pieces(), [a, c, []], [b, b, b])
    assert hyp_w[0] == ref_w[0] and len(hyp_w[0]) == 2
    assert MR.edit_distance(hyp_w[0], ref_w[0]) == 0         # two segmentations of the same words
    assert MR.edit_distance(a, b) == 3                       # unit token sees three different ids
    assert MR.edit_distance(hyp_w[1], ref_w[1]) == 1 and hyp_w[2] == [] and MR.edit_distance(hyp_w[2], ref_w[2]) == 2
    assert all(isinstance(w, int) and w > 0 for row in hyp_w + ref_w for w in row)


# ---- the end-to-end case is not degenerate ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MR.E2E_CASES)
def test_end_to_end_case_has_spread_weights(case):
    r = MR.criterion(case)
    p, err, count = r["p"], r["err"], r["count"]
    print(case, "p", p.T.tolist(), "err", err.T.tolist(), "count", count, "loss", r["loss"], "mwer", r["mwer"])
    assert count == [3, 2, 1]
    for u, n in enumerate(count):
        if n < 2:
            continue                                   # the empty list holds one hypothesis: p = 1 by definition
        assert p[:n, u].max() < 0.9
        assert len(set(err[:n, u].tolist())) >= 2
    assert abs(r["mwer"]) > 1e-3 and np.isfinite(r["loss"])
    assert all(np.isfinite(g).all() for g in r["grads"].values())
