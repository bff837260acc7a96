"""GPU: MWER training - the kernels (asrk_seq_logp_lse_f32, asrk_seq_logp_bwd_f32, asrk_mwer_loss_f64) against float64
on the same inputs, ASR.hypothesis_logp + MWERLoss end to end against the float64 oracle (tests/mwer_reference.py), the
search wrapper and the training solver.

Tolerances follow tests/test_rescore_gpu.py: E is the error of the existing differentiable path (ops.log_softmax +
gather, through autograd) on the same case, the new kernel must be within 2 * max(E, floor) with the floor
2^-23 * 80 forward and 2^-23 * max|w| backward - never derived from the new kernels' results."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mwer_reference as MR
from conftest import PKG_NAME
from helpers import CASES, load_golden, golden_state_dict, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


# ---- seq_logp_lse and its backward ---------------------------------------------------------------------------------------
def _strided(x, ld, offset, fill=0.0):
    """x [M,V] on the device with row stride ld, its base `offset` floats behind a 256-byte boundary -> (view, buffer)"""
    M, V = x.shape
    buf = torch.full((M * ld + offset + 4,), fill, dtype=torch.float32, device=DEV)
    view = buf[offset:offset + M * ld].view(M, ld)[:, :V]
    view.copy_(x)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view, buf


def _case(M):
    """targets with a skipped row, segments with an empty one and rows outside every segment"""
    if M == 1:
        return [[2], [0, 0, 1]], [[-1], [0, 1]], [[1], [1, 1]]            # live / skipped / outside every segment
    if M == 5:
        return [[1, -1, 0, 2, 1], [1, 3, 3, 4]],
    return [[0, 1, -1, 2, 0, 1, 2, -1, 1], [1, 4, 4, 8]],


@pytest.mark.parametrize("V", [3, 63, 64, 65, 1000, 2047, 2048, 2049, 4099])
@pytest.mark.parametrize("M", [1, 5, 9])
@pytest.mark.parametrize("pad,offset", [(0, 0), (3, 0), (0, 1), (1, 0)])
def test_seq_logp_lse_and_backward_against_float64(ops, V, M, pad, offset):
    """every variant: a wave per row (V < 2048) and a workgroup per row, 16-byte accesses (aligned base, stride % 4 == 0)
    and scalar ones; logits scaled to +-80; dx out of place with a stride of its own and in place"""
    L = _mod("_lib").load()
    g = torch.Generator().manual_seed(V * 31 + M * 7 + pad + offset)
    for tg_mod, seg in _case(M):
        x = (torch.rand((M, V), generator=g) * 2 - 1) * 80.0
        tgt = torch.tensor([t if t < 0 else int(torch.randint(0, V, (1,), generator=g)) for t in tg_mod])
        R = len(seg) - 1
        w = (torch.rand((R,), generator=g, dtype=torch.float64) * 2 - 1) * 3.0
        ld = V + pad
        xd, xbuf = _strided(x, ld, offset)
        tgt_d, seg_d, w_d = tgt.to(DEV), torch.tensor(seg, dtype=torch.int64, device=DEV), w.to(DEV)
        tok = torch.empty((M,), dtype=torch.float32, device=DEV)
        lse = torch.empty((M,), dtype=torch.float32, device=DEV)
        seq = torch.empty((R,), dtype=torch.float64, device=DEV)
        st = ops._stream()
        assert L.asrk_seq_logp_lse_f32(_p(xd), ld, _p(tgt_d), _p(seg_d), M, V, R, 0, _p(tok), _p(lse), _p(seq), st) == 0
        # forward: ops.seq_logp bit for bit
        tok0, seq0 = ops.seq_logp(xd, tgt_d, seg_d)
        assert torch.equal(tok, tok0) and torch.equal(seq, seq0)
        # float64 reference with autograd
        x64 = x.double().requires_grad_(True)
        tok_r, seq_r, lse_r = MR.seq_logp(x64, tgt, seg)
        ((seq_r * w).sum() + 0.0 * x64.sum()).backward()        # (the second term: a graph even when no row counts)
        live = (tgt >= 0).numpy()
        # E: the existing differentiable path on the same case
        xg = x.to(DEV).requires_grad_(True)
        roww = torch.zeros((M,), dtype=torch.float64)
        for r in range(R):
            roww[seg[r]:seg[r + 1]] = w[r]
        base = ops.log_softmax(xg)[torch.arange(M, device=DEV), tgt.clamp(min=0).to(DEV)]
        (base * (roww * torch.from_numpy(live)).float().to(DEV)).sum().backward()
        E_f = float((base.detach().cpu().double() - tok_r.detach())[torch.from_numpy(live)].abs().max()) if live.any() \
            else 0.0
        E_b = float((xg.grad.cpu().double() - x64.grad).abs().max())
        tol_f = 2 * max(E_f, 2.0 ** -23 * 80.0)
        tol_b = 2 * max(E_b, 2.0 ** -23 * float(w.abs().max()))
        err_tok = float((tok.cpu().double() - tok_r.detach()).abs().max())
        err_lse = float((lse.cpu().double() - lse_r.detach()).abs().max())
        assert all(float(tok[m]) == 0.0 and float(lse[m]) == 0.0 for m in range(M) if not live[m])
        assert err_tok <= tol_f and err_lse <= tol_f
        # backward, out of place: NaN-filled dx with its own stride
        ldd = ld + 4                        # the same alignment class as x: the 16-byte variant stays one
        dxd, dbuf = _strided(torch.full((M, V), float("nan")), ldd, offset, fill=float("nan"))
        assert L.asrk_seq_logp_bwd_f32(_p(xd), ld, _p(tgt_d), _p(lse), _p(seg_d), _p(w_d), M, V, R, _p(dxd), ldd,
                                       st) == 0
        got = dxd.cpu().double()
        err_b = float((got - x64.grad).abs().max())
        if (pad, offset) == (0, 0):         # an odd dx stride beside an aligned x: scalar accesses, the same values
            odd, _ = _strided(torch.full((M, V), float("nan")), ld + 1, 0, fill=float("nan"))
            assert L.asrk_seq_logp_bwd_f32(_p(xd), ld, _p(tgt_d), _p(lse), _p(seg_d), _p(w_d), M, V, R, _p(odd),
                                           ld + 1, st) == 0
            assert torch.equal(odd, dxd)
        zero_rows = [m for m in range(M) if not live[m] or not any(seg[r] <= m < seg[r + 1] for r in range(R))]
        assert zero_rows or M == 1
        for m in zero_rows:
            assert bool((dxd[m] == 0).all()), (m, "a skipped row must be written as exact zeros")
        # nothing but the [M, V] elements was written: the padding columns and the slack keep their NaN
        mask = torch.ones_like(dbuf, dtype=torch.bool)
        mask[offset:offset + M * ldd].view(M, ldd)[:, :V] = False
        assert bool(torch.isnan(dbuf[mask]).all())
        # in place: the same values
        assert L.asrk_seq_logp_bwd_f32(_p(xd), ld, _p(tgt_d), _p(lse), _p(seg_d), _p(w_d), M, V, R, _p(xd), ld,
                                       st) == 0
        ops.check_errors()
        assert torch.equal(xd, dxd)
        if pad:
            assert bool((xbuf[offset:offset + M * ld].view(M, ld)[:, V:] == 0).all())     # padding untouched
        print("V", V, "M", M, "ld", ld, "ldd", ldd, "offset", offset, "E_fwd", E_f, "err_tok", err_tok, "err_lse",
              err_lse, "tol", tol_f, "| E_bwd", E_b, "err_bwd", err_b, "tol", tol_b)
        assert err_b <= tol_b


def test_seq_logp_fn_autograd(ops):
    g = torch.Generator().manual_seed(3)
    M, V = 12, 257
    x = torch.randn((M, V), generator=g) * 4
    tgt = torch.randint(0, V, (M,), generator=g)
    tgt[5] = -1
    seg = torch.tensor([0, 4, 4, 12])
    w = torch.tensor([1.5, 7.0, -0.25], dtype=torch.float64)
    x64 = x.double().requires_grad_(True)
    _, seq_r, _ = MR.seq_logp(x64, tgt, seg.tolist())
    (seq_r * w).sum().backward()
    outs = []
    for inplace in (False, True):
        xg = x.to(DEV).requires_grad_(True)
        logits = xg * 1.0                                        # a non-leaf the in-place variant may write over
        seq = ops.SeqLogpFn.apply(logits, tgt.to(DEV), seg.to(DEV), inplace)
        assert seq.dtype == torch.float64 and torch.equal(seq, ops.seq_logp(xg.detach(), tgt, seg)[1])
        (seq * w.to(DEV)).sum().backward()
        outs.append(xg.grad.clone())
        # p = exp(x - lse): x - lse carries the roundings of x and lse (2^-24 of each), exp one more
        assert float((xg.grad.cpu().double() - x64.grad).abs().max()) <= 7.0 * 2.0 ** -23 * (2 + 2 * float(x.abs().max()))
        assert bool((xg.grad[5] == 0).all())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("V", [65, 2049])
def test_a_label_beyond_the_vocabulary_is_nan_forward_and_backward(ops, V):
    """target >= V: nothing is read; the token, its sequence and that row's gradient are NaN (a NaN score hands on a
    NaN gradient, as autograd would), every other row keeps its values"""
    L = _mod("_lib").load()
    g = torch.Generator().manual_seed(V)
    M = 6
    x = torch.randn((M, V), generator=g) * 4
    tgt = torch.randint(0, V, (M,), generator=g)
    seg = torch.tensor([0, 3, 5])                               # row 5 lies in no segment
    w = torch.tensor([2.0, -1.0], dtype=torch.float64)
    bad = tgt.clone()
    bad[1], bad[5] = V, V + 7

    def run(t):
        xd = x.to(DEV)
        tok, lse = (torch.empty((M,), dtype=torch.float32, device=DEV) for _ in range(2))
        seq = torch.empty((2,), dtype=torch.float64, device=DEV)
        dx = torch.full((M, V), 7.0, device=DEV)
        st = ops._stream()
        assert L.asrk_seq_logp_lse_f32(_p(xd), V, _p(t.to(DEV)), _p(seg.to(DEV)), M, V, 2, 0, _p(tok), _p(lse), _p(seq),
                                       st) == 0
        assert L.asrk_seq_logp_bwd_f32(_p(xd), V, _p(t.to(DEV)), _p(lse), _p(seg.to(DEV)), _p(w.to(DEV)), M, V, 2,
                                       _p(dx), V, st) == 0
        ops.check_errors()
        return tok.cpu(), lse.cpu(), seq.cpu(), dx.cpu()
    tok0, lse0, seq0, dx0 = run(tgt)
    tok, lse, seq, dx = run(bad)
    assert np.array_equal(tok.numpy(), ops.seq_logp(x.to(DEV), bad, seg)[0].cpu().numpy(), equal_nan=True)
    assert bool(torch.isnan(tok[[1, 5]]).all()) and lse[1] == 0 and lse[5] == 0
    assert bool(torch.isnan(seq[0])) and seq[1] == seq0[1]
    assert bool(torch.isnan(dx[1]).all())                       # in a segment: NaN
    assert bool((dx[5] == 0).all())                             # in no segment: zeros, like any such row
    keep = [0, 2, 3, 4]
    assert torch.equal(tok[keep], tok0[keep]) and torch.equal(dx[keep], dx0[keep])


# ---- mwer_loss -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 5, 32])
@pytest.mark.parametrize("U", [1, 3, 70])
@pytest.mark.parametrize("spread", [0.0, 1.0, 300.0])
def test_mwer_loss_against_float64(ops, N, U, spread):
    g = torch.Generator().manual_seed(N * 100 + U)
    s = -20.0 + spread * torch.rand((N, U), generator=g, dtype=torch.float64)
    err = torch.randint(0, 60, (N, U), generator=g, dtype=torch.int32)
    count = torch.randint(0, N + 1, (U,), generator=g, dtype=torch.int32)
    count[0] = N
    if U > 1:
        count[1] = 0
    if U > 2:
        count[2] = 1
    s_ref = s.clone().requires_grad_(True)
    loss_r, ee_r, _ = MR.mwer_loss(s_ref, err.numpy(), count.tolist())
    wu = torch.rand((U,), generator=g, dtype=torch.float64) + 0.5
    (loss_r * wu).sum().backward()
    sd = s.to(DEV).requires_grad_(True)
    loss, ee = ops.MWERLossFn.apply(sd, err.to(DEV), count.to(DEV))
    (loss * wu.to(DEV)).sum().backward()
    ops.check_errors()
    assert loss.dtype == ee.dtype == sd.grad.dtype == torch.float64
    close = lambda a, b: float((a.cpu() - b.detach()).abs().max()) <= 1e-12 * max(1.0, float(b.detach().abs().max()))
    assert close(loss, loss_r) and close(ee, ee_r) and close(sd.grad, s_ref.grad)
    valid = torch.arange(N).unsqueeze(1) < count.unsqueeze(0)
    assert bool((sd.grad.cpu()[~valid] == 0).all())
    for u in range(U):
        if count[u] <= 1:
            assert float(loss[u]) == 0.0 and bool((sd.grad[:, u] == 0).all())
    assert float(ee[1] if U > 1 else 0.0) == 0.0


def test_mwer_loss_fn_refuses_more_than_32_hypotheses(ops):
    """(the C entry points' argument checks are asserted once, in tests/test_mwer_cpu.py)"""
    with pytest.raises(_mod("_lib").AsrkError, match="shape"):
        ops.MWERLossFn.apply(torch.zeros((33, 2), dtype=torch.float64, device=DEV),
                             torch.zeros((33, 2), dtype=torch.int32, device=DEV),
                             torch.ones((2,), dtype=torch.int32, device=DEV))


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _model(case):
    g = load_golden(case)
    cfg, D, V = CASES[case][0], CASES[case][1], CASES[case][2]
    model = _mod("src.asr").ASR(D, V, True, cfg["ctc_weight"], cfg["encoder"], cfg["attention"] or {},
                                cfg["decoder"] or {})
    model.load_state_dict(golden_state_dict(g), strict=True)
    return cfg, D, V, model.to(DEV)


def _base_loss(ops, model, ctc_out, enc_len, att_out, txt):
    txt_len = torch.sum(txt != 0, dim=-1)
    total = 0
    if ctc_out is not None:
        total = total + ops.CTCLoss(blank=0)(ctc_out.transpose(0, 1), txt, enc_len, txt_len) * model.ctc_weight
    b, t, _ = att_out.shape
    return total + ops.CrossEntropyLoss(ignore_index=0)(att_out.view(b * t, -1), txt.view(-1)) * (1 - model.ctc_weight)


@pytest.mark.parametrize("case", MR.E2E_CASES)
def test_mwer_step_end_to_end_against_the_oracle(ops, case):
    """fixed synthetic lists (no search: ties cannot move the test); loss and every parameter gradient against the
    float64 oracle within 1e-3, the stricter of the training-step bounds of tests/test_model_gpu.py (measured on an
    MI355X: the largest gradient error is 6.4e-6 / 1.9e-5 / 7.6e-6 on the three models)"""
    M = _mod("src.mwer")
    ref = MR.criterion(case)
    cfg, D, V, model = _model(case)
    model.train()
    fused = _mod("speller_ops").supported_train_loop(model.attention, model.decoder, True)
    assert fused == (case == "las_hybrid_loc")               # both loops of hypothesis_logp are covered
    feat, flen, txt, lists = MR.e2e_inputs(case)
    opts = M.MWEROptions(nbest=MR.NBEST, beam_size=MR.NBEST, ce_weight=MR.CE_WEIGHT, unit='token')
    crit = M.MWERLoss(model, None, opts)
    nbest = M.pack_nbest(lists, MR.NBEST)
    assert nbest[2].tolist() == ref["count"]
    txt_d = txt.to(DEV)
    enc, enc_len0 = model.encoder(feat.to(DEV), flen.to(DEV))
    ctc_out, enc_len, att_out, _, _ = model(feat.to(DEV), flen.to(DEV), int((txt != 0).sum(-1).max()), tf_rate=1.0,
                                            teacher=txt_d, encoded=(enc, enc_len0))
    base = _base_loss(ops, model, ctc_out, enc_len, att_out, txt_d)
    s = model.hypothesis_logp(enc, enc_len, nbest[0].to(DEV), nbest[1].to(DEV))
    assert s.dtype == torch.float64 and model.training
    print(case, "s", s.tolist(), "oracle", ref["s"].tolist())
    assert rel_err(s.detach().cpu(), ref["s"]) < 1e-3
    mwer, stats = crit(nbest, enc, enc_len, txt)
    total = mwer.to(torch.float32) + MR.CE_WEIGHT * base
    total.backward()
    ops.check_errors()
    print(case, "mwer", float(mwer), ref["mwer"], "base", float(base), ref["base"], "total", float(total), ref["loss"],
          "stats", float(stats['exp_err']), ref["exp_err"], float(stats['best_err']), ref["best_err"])
    assert torch.equal(enc_len.cpu(), ref["enc_len"])
    assert abs(float(mwer) - ref["mwer"]) < 1e-3 * abs(ref["mwer"])
    assert abs(float(total) - ref["loss"]) < 1e-3 * abs(ref["loss"])
    assert abs(float(stats['exp_err']) - ref["exp_err"]) < 1e-3 * ref["exp_err"]
    assert abs(float(stats['best_err']) - ref["best_err"]) <= 1e-12       # a mean of integers
    worst = ("", 0.0)
    for n, p in model.named_parameters():
        if np.max(np.abs(ref["grads"][n])) < 1e-7:
            # tests/test_model_gpu.py's rule: a gradient that is rounding alone has no relative error (gen_energy.bias:
            # the softmax does not see it); it must still be as small here
            assert float(p.grad.abs().max()) < 1e-6, n
            continue
        e = rel_err(p.grad.cpu(), ref["grads"][n])
        worst = max(worst, (n, e), key=lambda t: t[1])
        assert e < 1e-3, (n, e)
    print(case, "largest gradient error", worst)


def test_error_counts_in_words_and_tokens(ops):
    _Pieces = MR.Pieces
    M = _mod("src.mwer")
    a, b, c = [3, 4, 6], [5, 7, 8], [5, 9]          # hello world / hello world / hello there
    hyps, refs = [a, [6], c, b, [], [9]], [b, [9]]   # N = 3 rows per utterance, row n * 2 + u
    words = M.error_counts(_Pieces(), hyps, refs, 'word', DEV)
    tokens = M.error_counts(None, hyps, refs, 'token', DEV)
    assert words.dtype == tokens.dtype == torch.int32 and words.is_cuda
    assert words.tolist() == [0, 1, 1, 2, 2, 0]     # two segmentations of the same words: distance 0
    assert tokens.tolist() == [3, 1, 2, 3, 3, 0]
    assert tokens.tolist() == [MR.edit_distance(h, refs[r % 2]) for r, h in enumerate(hyps)]
    with pytest.raises(ValueError):
        M.error_counts(None, hyps, refs, 'char', DEV)


# ---- the search wrapper ------------------------------------------------------------------------------------------------------
def _fresh_lists(case, model, opts, feat, flen):
    """the top N of a fresh BeamDecoder on a copy of the weights, packed"""
    twin = _model(case)[3]
    twin.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()}, strict=True)
    twin.eval()
    dec = _mod("src.decode").BeamDecoder(twin, None, opts.beam_size, opts.min_len_ratio, opts.max_len_ratio,
                                         ctc_weight=opts.ctc_weight)
    with torch.no_grad():
        lists = dec.forward_batch(feat, flen)
    scores = [h.avgScore() for hyps in lists for h in hyps]
    return _mod("src.mwer").pack_nbest([[h.outIndex for h in hyps] for hyps in lists], opts.nbest), scores


# the device-resident batched search (with the joint CTC score) and the per-utterance forward() fallback (a two-layer
# GRU decoder; without CTC: the reference's own beam search raises on this random-weight model with it)
@pytest.mark.parametrize("case,ctc_w,batched", [("las_hybrid_loc", 0.3, True), ("las_gru", 0.0, False)])
def test_nbest_search_follows_the_weights(ops, case, ctc_w, batched):
    import rescore_cases as RC
    M = _mod("src.mwer")
    cfg, D, V, model = _model(case)
    model.train()
    feat, flen = RC.utterances(case, D)
    feat, flen = feat.to(DEV), flen.to(DEV)
    opts = M.MWEROptions(nbest=3, beam_size=4, unit='token', ctc_weight=ctc_w, max_len_ratio=0.3)
    search = M.NBestSearch(model, opts)
    assert search.decoder.batchable() == batched
    assert any("host-driven" in m for m in search.create_msg()) == (not batched)
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]
    scores_of = lambda: [h.avgScore() for hyps in search.last_hyps for h in hyps]
    close = lambda a, b: len(a) == len(b) and all(abs(x - y) <= 1e-5 * max(1.0, abs(y)) for x, y in zip(a, b))
    got = search(feat, flen)
    s0 = scores_of()
    assert model.training and model.attention.key is None
    fresh, fresh_scores = _fresh_lists(case, model, opts, feat, flen)
    assert same(got, fresh) and close(s0, fresh_scores)
    assert got[0].shape[0] == 3 * 3 and int(got[2].max()) <= 3
    # one optimiser step through the fused update (raw-pointer writes), then again: the scores must MOVE, by far more
    # than the tolerance they are compared with, and be those of a fresh decoder on the updated weights
    opt = _mod("src.optim").Optimizer([{'params': model.parameters()}], optimizer='Adadelta', lr=1.0, eps=1e-2,
                                      lr_scheduler='fixed')
    assert opt.fused
    opt.pre_step(0)
    g = load_golden(case)
    txt = torch.from_numpy(g["txt"]).to(DEV)
    ctc_out, enc_len, att_out, _, _ = model(torch.from_numpy(g["feat"]).to(DEV), torch.from_numpy(g["feat_len"]).to(DEV),
                                            int((txt != 0).sum(-1).max()), tf_rate=1.0, teacher=txt)
    before = [p.detach().clone() for p in model.parameters()]
    _base_loss(ops, model, ctc_out, enc_len, att_out, txt).backward()
    opt.step()
    assert any(bool((a != b).any()) for a, b in zip(before, model.parameters()))
    again = search(feat, flen)
    s1 = scores_of()
    ops.check_errors()
    assert model.training
    fresh, fresh_scores = _fresh_lists(case, model, opts, feat, flen)
    moved = max(abs(a - b) for a, b in zip(s0, s1)) if len(s0) == len(s1) else float("inf")
    print(case, "scores before", s0[:4], "after", s1[:4], "moved by", moved)
    assert moved > 1e-3
    assert same(again, fresh) and close(s1, fresh_scores)


# ---- the solver ----------------------------------------------------------------------------------------------------------------
def test_solver_with_and_without_the_block(tmp_path):
    out = str(tmp_path / "mwer.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "mwer_worker.py"), out], capture_output=True, text=True,
                       env=dict(os.environ, ASRK_DETERMINISTIC="1"), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    plain, off, late, on = res["plain"], res["off"], res["late"], res["on"]
    # without the block, with enable: false, and before start_step: the same step, bit for bit
    assert plain["mwer_logs"] == [] and off["mwer_logs"] == [] and late["mwer_logs"] == []
    assert plain["loss_hex"] == off["loss_hex"] == late["loss_hex"] and plain["param_sha1"] == off["param_sha1"]
    assert plain["param_sha1"] == late["param_sha1"]
    assert not plain["has_search"] and not off["has_search"] and late["has_search"]
    # start_step 1: step 0 is the plain step, step 1 carries the MWER entries
    assert on["loss_hex"][0] == plain["loss_hex"][0]
    assert on["loss_hex"][1] != plain["loss_hex"][1]
    assert on["searches"] == len(on["loss_hex"]) - 1 and plain["searches"] == 0
    assert len(on["mwer_logs"]) >= 1
    for entry in on["mwer_logs"]:
        assert set(entry) == {"tr_exp_err", "tr_1best_err"}
        assert all(np.isfinite(v) and v >= 0 for v in entry.values())
    assert all(np.isfinite(v) for v in on["grad_norm"]) and on["params_finite"]
    assert on["param_sha1"] != plain["param_sha1"]
    assert any("MWER" in m for m in on["msgs"])
