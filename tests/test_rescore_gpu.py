"""GPU: the two second-pass kernels (ops.seq_logp, ops.ctc_score_rows; csrc/rescore.hip) against float64 on the same f32
inputs, and RescoreDecoder end to end on golden models against tests/rescore_reference.py driven by the CPU oracle.

Measured on an MI355X: the tolerances below are derived from the existing paths' own error, never
from the new kernels' results."""
import importlib

import numpy as np
import pytest
import torch

import rescore_cases as RC
import rescore_reference as RR
from conftest import PKG_NAME
from helpers import CASES, load_golden, golden_state_dict
from oracle import asr_oracle as AO

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


# ---- seq_logp -----------------------------------------------------------------------------------------------------------
def _strided(x, ldx, offset):
    """x [M,V] on the device with row stride ldx, its base `offset` floats behind a 256-byte boundary"""
    M, V = x.shape
    buf = torch.zeros((M * ldx + offset + 4,), dtype=torch.float32, device=DEV)
    view = buf[offset:offset + M * ldx].view(M, ldx)[:, :V]
    view.copy_(x)
    assert view.data_ptr() % 16 == (4 * offset) % 16 and view.stride(0) == ldx
    return view


@pytest.mark.parametrize("V", [1, 3, 63, 64, 65, 255, 257, 1000, 4099])
@pytest.mark.parametrize("pad,offset", [(0, 0), (3, 0), (0, 1), (1, 0)])
def test_seq_logp_against_float64(ops, V, pad, offset):
    """every variant: one wave per row (V < 2048) and one workgroup per row (4099), 16-byte loads (ldx % 4 == 0 and an
    aligned base) and scalar loads (odd ldx, or the base moved by one float); logits scaled to +-80"""
    M = 37
    g = torch.Generator().manual_seed(V * 7 + pad + offset)
    x = (torch.rand((M, V), generator=g) * 2 - 1) * 80.0
    tgt = torch.randint(0, V, (M,), generator=g)
    ldx = V + pad
    if V > 1:
        x[3] = float("-inf")
        x[3, tgt[3]] = 5.0                     # -inf everywhere but the target: 0
        x[4, tgt[4]] = float("-inf")           # the target's logit is -inf: -inf
        x[5, (tgt[5] + 1) % V] = float("-inf")
    xd = _strided(x, ldx, offset)
    want = RR.seq_logp(x.numpy(), tgt.numpy())
    base = ops.log_softmax(x.to(DEV)).cpu().double().numpy()[np.arange(M), tgt.numpy()]
    fin = np.isfinite(want)
    E = float(np.abs(base[fin] - want[fin]).max())
    tol = 2 * max(E, 2.0 ** -23 * 80.0)
    tok, seq = ops.seq_logp(xd, tgt)
    ops.check_errors()
    assert seq is None
    got = tok.cpu().double().numpy()
    err = float(np.abs(got[fin] - want[fin]).max())
    print("V", V, "ldx", ldx, "offset", offset, "E(log_softmax + gather)", E, "err(seq_logp)", err, "tol", tol)
    assert np.array_equal(got[~fin], want[~fin])
    if V > 1:
        assert got[3] == 0.0 and got[4] == -np.inf
    assert err <= tol


def test_seq_logp_skipped_rows_bad_targets_normalized_and_sums(ops):
    V, M = 257, 40
    g = torch.Generator().manual_seed(5)
    x = torch.randn((M, V), generator=g) * 3
    tgt = torch.randint(0, V, (M,), generator=g)
    seg = torch.tensor([0, 7, 7, 20, 40])                       # an empty segment among them
    tok0, seq0 = ops.seq_logp(x.to(DEV), tgt, seg)
    skip = [2, 9, 39]
    x2, tgt2 = x.clone(), tgt.clone()
    x2[skip] = float("nan")
    tgt2[skip] = -1
    tgt2[11] = V                                                # out of range: NaN in that row only
    tok, seq = ops.seq_logp(x2.to(DEV), tgt2, seg)
    ops.check_errors()
    tok, tok0 = tok.cpu().numpy(), tok0.cpu().numpy()
    assert all(tok[m] == 0.0 for m in skip) and np.isnan(tok[11])
    keep = [m for m in range(M) if m not in skip + [11]]
    assert np.array_equal(tok[keep], tok0[keep])                # no other result changes
    # the sums are the sequential float64 sums of the returned tokens, bit for bit
    for t_, s_, off in ((tok0, seq0, seg), (tok, seq, seg)):
        want = []
        for r in range(len(off) - 1):
            acc = np.float64(0.0)
            for m in range(int(off[r]), int(off[r + 1])):
                acc = acc + np.float64(t_[m])
            want.append(acc)
        got = s_.cpu().numpy()
        assert got.dtype == np.float64 and got[1] == 0.0
        assert np.array_equal(got, np.asarray(want), equal_nan=True)
    one = ops.seq_logp(x.to(DEV), tgt, torch.tensor([0, M]))[1].cpu().numpy()      # R = 1
    acc = np.float64(0.0)
    for m in range(M):
        acc = acc + np.float64(tok0[m])
    assert one.shape == (1,) and one[0] == acc
    # normalized: the gathered value, bit for bit (4099: the workgroup variant)
    for Vn in (257, 4099):
        xn = torch.randn((9, Vn), generator=g)
        tn = torch.randint(0, Vn, (9,), generator=g)
        got = ops.seq_logp(xn.to(DEV), tn, normalized=True)[0].cpu().numpy()
        assert np.array_equal(got, xn.numpy()[np.arange(9), tn.numpy()])
    empty = ops.seq_logp(torch.zeros((0, 5), device=DEV), torch.zeros((0,), dtype=torch.int64))
    assert empty[0].shape == (0,)


# ---- ctc_score_rows -----------------------------------------------------------------------------------------------------
def _ctc_case(ops, lp, mem_len, rows, V, T_floor):
    """rows: (utterance, targets); lp [U,Tmax,V] with NaN beyond mem_len.  Reference: -ctc_numpy in float64; tolerance
    from the error of ops.CTCLoss(reduction='none') on the same rows with the posteriors repeated per row."""
    R = len(rows)
    Lmax = max(1, max(len(y) for _, y in rows))
    tg = np.zeros((R, Lmax), dtype=np.int64)
    for r, (_, y) in enumerate(rows):
        tg[r, :len(y)] = y
    tl = [len(y) for _, y in rows]
    rm = [u for u, _ in rows]
    got = ops.ctc_score_rows(lp.to(DEV), mem_len, rm, tg, tl).cpu().double().numpy()
    ops.check_errors()
    with np.errstate(all='ignore'):
        want = np.array([-AO.ctc_numpy(lp[u, :mem_len[u]].numpy()[:, None, :], [y], [mem_len[u]], [len(y)])[0]
                         for u, y in rows])
    Tmax = lp.shape[1]
    rep = torch.zeros((Tmax, R, V))
    for r, (u, _) in enumerate(rows):
        rep[:mem_len[u], r] = lp[u, :mem_len[u]]
    loss = ops.CTCLoss(reduction='none')(rep.to(DEV), torch.from_numpy(tg), [mem_len[u] for u in rm], tl)
    base = -loss.cpu().double().numpy()
    fin = np.isfinite(want)
    E = float(np.abs(base[fin] - want[fin]).max())
    tol = 2 * max(E, T_floor * 2.0 ** -22)
    err = float(np.abs(got[fin] - want[fin]).max())
    print("rows", R, "Tmax", Tmax, "E(CTCLoss)", E, "err(ctc_score_rows)", err, "tol", tol)
    assert np.array_equal(got[~fin], want[~fin]), (got, want)
    assert err <= tol
    return got


def _posteriors(seed, lens, V, Tmax):
    g = torch.Generator().manual_seed(seed)
    lp = torch.full((len(lens), Tmax, V), float("nan"))
    for u, T in enumerate(lens):
        lp[u, :T] = torch.log_softmax(torch.randn((T, V), generator=g) * 2, -1)
    return lp


def test_ctc_score_rows_short_targets_interleaved_rows(ops):
    V, lens = 11, [1, 7, 40]
    lp = _posteriors(1, lens, V, 40)
    four = _posteriors(2, [4, 3], V, 4)
    rows = [(2, [3, 3, 5]), (0, []), (1, [4]), (2, []), (0, [2]), (1, [2, 2]), (2, [9]), (1, []), (0, [1, 2]),
            (1, [1, 2, 3]), (2, [7, 8]), (1, [5, 5, 5, 5, 5]), (2, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])]
    got = _ctc_case(ops, lp, lens, rows, V, 40)
    assert got[8] == -np.inf                       # two labels on one frame
    assert got[11] == -np.inf                      # 5 repeats need 9 frames, the utterance has 7
    assert np.isfinite(got[[0, 1, 2, 3, 4, 6, 9, 10, 12]]).all()
    rep = _ctc_case(ops, four, [4, 3], [(0, [6, 6, 2]), (1, [6, 6, 2])], V, 4)
    assert np.isfinite(rep[0]) and rep[1] == -np.inf      # a a b: finite on 4 frames, impossible on 3
    # a bad label and a bad row_mem: NaN in those rows only
    tg = np.zeros((len(rows), 10), dtype=np.int64)
    for r, (_, y) in enumerate(rows):
        tg[r, :len(y)] = y
    tl = [len(y) for _, y in rows]
    rm = [u for u, _ in rows]
    tg2, rm2 = tg.copy(), list(rm)
    tg2[6, 0] = V
    rm2[2] = 3
    rm2[7] = -1
    bad = ops.ctc_score_rows(lp.to(DEV), lens, rm2, tg2, tl).cpu().double().numpy()
    ops.check_errors()
    assert np.isnan(bad[[2, 6, 7]]).all()
    keep = [r for r in range(len(rows)) if r not in (2, 6, 7)]
    assert np.array_equal(bad[keep], got[keep])


def test_ctc_score_rows_states_across_the_64_lanes(ops):
    """tgt_len 31, 32, 33 on 80 frames: S = 63, 65, 67 (one and two states per lane)"""
    V = 11
    lp = _posteriors(3, [80, 80], V, 80)
    g = np.random.RandomState(0)
    rows = [(r % 2, list(g.randint(1, V, size=n))) for r, n in enumerate([31, 32, 33, 33, 31])]
    got = _ctc_case(ops, lp, [80, 80], rows, V, 80)
    assert np.isfinite(got).all()


def test_ctc_score_rows_long_lattice_takes_the_library_functions(ops):
    """T = 520 > 512: the library expf / logf path"""
    V = 11
    lp = _posteriors(4, [520, 100], V, 520)
    got = _ctc_case(ops, lp, [520, 100], [(0, [1, 2, 3, 4, 5]), (1, [5, 4]), (0, [])], V, 520)
    assert np.isfinite(got).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _model(case):
    g = load_golden(case)
    cfg, D, V = CASES[case][0], CASES[case][1], CASES[case][2]
    model = _mod("src.asr").ASR(D, V, True, cfg["ctc_weight"], cfg["encoder"], cfg["attention"] or {},
                                cfg["decoder"] or {})
    model.load_state_dict(golden_state_dict(g), strict=True)
    return g, cfg, D, V, model.to(DEV).eval()


def _decoder(model, **kw):
    a = dict(beam_size=RC.BEAM, vocab_candidate=RC.CAND, ctc_weight=RC.CTC_W, device=DEV)
    a.update(kw)
    return _mod("src.rescore").RescoreDecoder(model, **a)


@pytest.mark.parametrize("case", RC.E2E_CASES)
def test_rescore_end_to_end_against_the_oracle(ops, case):
    g, cfg, D, V, model = _model(case)
    feat, flen = RC.utterances(case, D)
    dec = _decoder(model)
    first = _mod("src.ctc").CTCBeamDecoder(model, RC.vocab_range(V), RC.BEAM, RC.CAND, device=DEV)
    sd64 = RR.f64_state_dict(golden_state_dict(g))
    sd32 = golden_state_dict(g)
    alone = []
    for u in range(feat.shape[0]):
        f1, l1 = feat[u:u + 1, :int(flen[u])].contiguous(), flen[u:u + 1]
        res = dec(f1.to(DEV), l1.to(DEV))
        ops.check_errors()
        alone.append(res)
        # the first-pass list is CTCBeamDecoder's, unchanged
        nbest = [list(y) for y in first(f1.to(DEV), l1.to(DEV))]
        by_first = sorted(res, key=lambda h: h.first_rank)
        assert [list(h.tokens) for h in by_first] == nbest and [h.first_rank for h in by_first] == list(range(len(nbest)))
        assert all(h.outIndex == list(h.tokens) for h in res)
        # scores against the float64 oracle; tolerance: twice the gap of the existing teacher-forced GPU path to the
        # same oracle on the same inputs, plus the kernel tolerances
        s_ctc, s_att, lp64 = RR.acoustic_scores(sd64, cfg, f1, l1, nbest)
        Lmax = max(len(h) for h in nbest) + 1
        teacher = torch.zeros((len(nbest), Lmax), dtype=torch.long)
        for r, h in enumerate(nbest):
            teacher[r, :len(h)] = torch.tensor(h, dtype=torch.long)
            teacher[r, len(h)] = 1
        with torch.no_grad():
            ctc_g, _, att_g, _, _ = model(f1.to(DEV).repeat(len(nbest), 1, 1), l1.to(DEV).repeat(len(nbest)), Lmax,
                                          tf_rate=1.0, teacher=teacher.to(DEV))
            _, _, att_o, _, _ = AO.asr_forward(sd64, cfg, f1.double().repeat(len(nbest), 1, 1), l1.repeat(len(nbest)),
                                               Lmax, teacher=teacher)
        # the existing path's gap, measured where it is defined: the largest error of a logit / of a CTC log-prob.
        # A token's log-probability moves by at most twice the logit error (the logit and the log-sum-exp), a sum over
        # L tokens by L times that; a CTC path sums T log-probs.  On top, the kernels' own tolerances (above).
        gap_logit = float((att_g.cpu().double() - att_o).abs().max())
        gap_lp = float(np.abs(ctc_g[0].cpu().double().numpy() - lp64).max())
        T = lp64.shape[0]
        tol_att = 2 * (Lmax * 2 * gap_logit) + Lmax * 2 * 2.0 ** -23 * float(att_o.abs().max())
        tol_ctc = 2 * T * gap_lp + 2 * T * 2.0 ** -22
        for h in by_first:
            r = h.first_rank
            print(case, u, r, list(h.tokens), "ctc", h.ctc, s_ctc[r], "att", h.att, s_att[r], "tol", tol_ctc, tol_att)
        for h in by_first:
            r = h.first_rank
            assert abs(h.ctc - s_ctc[r]) <= tol_ctc or (h.ctc == s_ctc[r] == -np.inf)
            assert abs(h.att - s_att[r]) <= tol_att
            assert h.lm == 0.0
        scores = [RR.combine(c, a, 0.0, RC.CTC_W, 0.0) for c, a in zip(s_ctc, s_att)]
        order = RR.rank(scores)
        srt = [scores[i] for i in order]
        tol = RC.CTC_W * tol_ctc + (1 - RC.CTC_W) * tol_att
        print(case, u, "reference scores", srt, "tol", tol)
        assert all(a - b > 100 * tol for a, b in zip(srt, srt[1:]) if np.isfinite(b))   # decided by 100x the tolerance
        assert [h.first_rank for h in res] == order
        assert all(abs(h.score - scores[h.first_rank]) <= tol for h in res if np.isfinite(h.score))
        if u == 0:
            # the empty hypothesis (what an all-blank utterance's list [[]] holds), scored directly: the blank path
            # and p(<eos> | <sos>)
            enc, enc_len, frames = dec._encode(f1.to(DEV), l1.to(DEV))
            ctc_out = ops.log_softmax(ops.linear(enc, model.ctc_layer.weight, model.ctc_layer.bias))
            c0, a0, _ = dec.score_nbest(enc, enc_len, ctc_out, frames, [[[]]])
            e_ctc, e_att, _ = RR.acoustic_scores(sd64, cfg, f1, l1, [[]])
            print(case, "empty hypothesis", c0, e_ctc, a0, e_att)
            assert abs(c0[0] - e_ctc[0]) <= tol_ctc and abs(a0[0] - e_att[0]) <= tol_att
            ranked = _mod("src.rescore").rank_hypotheses([[]], c0, a0, None, RC.CTC_W, 0.0)
            assert len(ranked) == 1 and ranked[0].tokens == () and ranked[0].outIndex == []
    # the batch gives the same lists in the same order, and a small workspace (several chunks) the same bits
    batch = dec.forward_batch(feat.to(DEV), flen.to(DEV))
    ops.check_errors()
    assert [[(h.tokens, h.first_rank) for h in b] for b in batch] == [[(h.tokens, h.first_rank) for h in a] for a in alone]
    for a, b in zip(alone, batch):
        for x, y in zip(a, b):
            assert abs(x.score - y.score) <= 1e-4 * max(1.0, abs(x.score)) or x.score == y.score
    assert model.score_chunks == 1
    small = _decoder(model, workspace_mb=1e-3)
    again = small.forward_batch(feat.to(DEV), flen.to(DEV))
    ops.check_errors()
    assert model.score_chunks > 1
    assert again == batch                                              # bit-identical scores


def test_score_hypotheses_takes_an_empty_list(ops):
    g, cfg, D, V, model = _model("las_hybrid_loc")
    enc = torch.zeros((1, 5, model.encoder.out_dim), device=DEV)
    tok, s = model.score_hypotheses(enc, torch.tensor([5]), torch.zeros((0,), dtype=torch.int64),
                                    torch.zeros((0, 3), dtype=torch.int64), torch.zeros((0,), dtype=torch.int64))
    assert tok.shape == (0, 3) and s.shape == (0,)


# ---- with language models ---------------------------------------------------------------------------------------------
LM_W = 0.3


def _lstm_lm(tmp_path):
    """the `lm` golden configuration of oracle/gen_golden.py (lm_cases: the LSTM model, V = 13) as checkpoint + config"""
    import yaml
    z = load_golden("lm_train")
    cfg = dict(emb_tying=False, emb_dim=8, module='LSTM', dim=12, n_layers=2, dropout=0.0)
    sd = {k[len("lstm.param."):]: torch.from_numpy(v.copy()) for k, v in z.items() if k.startswith("lstm.param.")}
    ckpt, conf = str(tmp_path / "lm.pth"), str(tmp_path / "lm.yaml")
    torch.save({'model': sd}, ckpt)
    yaml.safe_dump({'model': cfg}, open(conf, 'w'))
    return ckpt, conf, cfg, sd


def _lm_reference(kind, tmp_path, V):
    """-> (lm_path, lm_config, f(y) -> (s_lm float64, per-token tolerance scale))"""
    import ngram_cases as NC
    import ngram_reference as NR
    if kind == "ngram":
        path = NC.joint_lm_arpa(tmp_path / "lm.arpa", V)
        m = NR.read_arpa(path, V)
        step = NR.f64_lm_step(m)

        def s_lm(y):
            st, acc, big = None, 0.0, 1.0
            for tok, tgt in zip([0] + list(y), list(y) + [1]):
                row, st = step(tok, st)
                acc += float(row[tgt])
                big += max(1.0, abs(float(row[tgt])))
            return acc, big - 1.0                                  # sum of the token magnitudes
        return path, '', s_lm, NC.JOINT_LM_ORDER
    ckpt, conf, cfg, sd = _lstm_lm(tmp_path)
    sd64 = RR.f64_state_dict(sd)

    def s_lm(y):
        inp = torch.tensor([[0] + list(y)], dtype=torch.long)
        with torch.no_grad():
            logits = AO.lm_forward(sd64, cfg, inp)[0].numpy()
        return float(sum(RR.seq_logp(logits, list(y) + [1]).tolist())), float(np.abs(logits).max())
    return ckpt, conf, s_lm, None


@pytest.mark.parametrize("first_pass_lm", [False, True])
@pytest.mark.parametrize("kind", ["rnn", "ngram"])
def test_rescore_with_a_language_model(ops, tmp_path, kind, first_pass_lm):
    case = "las_hybrid_loc"
    g, cfg, D, V, model = _model(case)
    lm_path, lm_config, s_lm, order_n = _lm_reference(kind, tmp_path, V)
    dec = _decoder(model, lm_path=lm_path, lm_config=lm_config, lm_weight=LM_W, first_pass_lm=first_pass_lm)
    assert any("LM rescoring" in line for line in dec.create_msg())
    feat, flen = RC.utterances(case, D, seed=RC.LM_SEED)
    sd64 = RR.f64_state_dict(golden_state_dict(g))
    plain = _decoder(model)
    changed = False
    for u in range(feat.shape[0]):
        f1, l1 = feat[u:u + 1, :int(flen[u])].contiguous(), flen[u:u + 1]
        res = dec(f1.to(DEV), l1.to(DEV))
        ops.check_errors()
        by_first = sorted(res, key=lambda h: h.first_rank)
        nbest = [list(h.tokens) for h in by_first]
        no_lm = sorted(plain(f1.to(DEV), l1.to(DEV)), key=lambda h: h.first_rank)
        if not first_pass_lm:
            assert nbest == [list(h.tokens) for h in no_lm]              # the first pass has no LM by default
        else:
            changed |= nbest != [list(h.tokens) for h in no_lm]
        s_ctc, s_att, lp64 = RR.acoustic_scores(sd64, cfg, f1, l1, nbest)
        want = [s_lm(y) for y in nbest]
        L = max(len(y) for y in nbest) + 1
        if kind == "ngram":
            # every token value is a sum of at most `order` f32 terms, each rounded once (relative 2^-24, allowed
            # twice), read back bit for bit and summed in float64
            tol_lm = max(order_n * 2.0 ** -23 * big for _, big in want)
        else:
            inp = torch.zeros((len(nbest), L), dtype=torch.long)
            for r, y in enumerate(nbest):
                inp[r, 1:1 + len(y)] = torch.tensor(y, dtype=torch.long)
            with torch.no_grad():
                got_logits = dec.lm(inp.to(DEV), torch.full((len(nbest),), L))[0].cpu().double()
            ref_logits = AO.lm_forward(RR.f64_state_dict(_lstm_lm(tmp_path)[3]), _lstm_lm(tmp_path)[2], inp)
            gap = float((got_logits - ref_logits.detach()).abs().max())
            # the kernel's own share, as in test_seq_logp_against_float64: E = error of log_softmax + gather on the
            # same f32 logits
            flat = got_logits.reshape(-1, V)
            E = float((ops.log_softmax(flat.float().to(DEV)).cpu().double()
                       - torch.from_numpy(RR.log_softmax(flat.numpy()))).abs().max())
            tol_lm = 2 * (L * 2 * gap) + L * 2 * max(E, 2.0 ** -23 * max(big for _, big in want))
        for h in by_first:
            print(kind, first_pass_lm, u, h.first_rank, list(h.tokens), "lm", h.lm, want[h.first_rank][0], "tol", tol_lm)
        assert all(abs(h.lm - want[h.first_rank][0]) <= tol_lm for h in by_first)
        scores = [RR.combine(c, a, l[0], RC.CTC_W, LM_W) for c, a, l in zip(s_ctc, s_att, want)]
        order = RR.rank(scores)
        srt = [scores[i] for i in order]
        gaps = [a - b for a, b in zip(srt, srt[1:]) if np.isfinite(b)]
        tol = max(abs(h.score - scores[h.first_rank]) for h in res if np.isfinite(h.score))
        print(kind, first_pass_lm, u, "reference scores", srt, "largest score error", tol, "lm tol", tol_lm)
        assert min(gaps) > 100 * LM_W * tol_lm and min(gaps) > 1e-3
        assert tol <= 1e-4                       # ctc / att parts are held to their own tolerances in the test above
        assert [h.first_rank for h in res] == order
    if first_pass_lm:
        assert changed                           # the fused first pass did produce another list somewhere


# ---- through main.py --test ----------------------------------------------------------------------------------------------
def test_rescore_through_main(tmp_path, monkeypatch):
    import os
    from test_e2e_gpu import _configs, _decode_cfg, _make_corpus
    from test_ctc_align_e2e_gpu import _seeded_checkpoint
    main = _mod("main")
    monkeypatch.delenv('ASRK_DECODE_BATCH', raising=False)
    tmp = str(tmp_path)
    root = os.path.join(tmp, 'corpus')
    vocab = _make_corpus(root)
    train, tr_path = _configs(root, vocab, tmp)
    ckpt = _seeded_checkpoint(tmp, train, vocab)
    result = os.path.join(tmp, 'result')
    common = ['--logdir', os.path.join(tmp, 'log'), '--ckpdir', os.path.join(tmp, 'ckpt'), '--outdir', result,
              '--njobs', '1', '--no-msg']
    kw = dict(beam_size=4, vocab_candidate=6, min_len_ratio=0.01, max_len_ratio=0.3, ctc_weight=0.3)
    rcfg = _decode_cfg(tmp, tr_path, ckpt, 'dec_rescore', rescore={'enable': True, 'workspace_mb': 64}, **kw)
    solver = main.main(['--config', rcfg, '--test'] + common)
    assert isinstance(solver.decoder, _mod("src.rescore").RescoreDecoder)
    names = sorted(os.listdir(result))
    assert names == ['dec_rescore_%s_%s.csv' % (s, k) for s in ('dev', 'test')
                     for k in ('beam-4-0.0', 'output', 'rescore-4-0.3-0.0')]
    for s, ds in (('dev', solver.dv_set), ('test', solver.tt_set)):
        rows = [l.split('\t') for l in open(os.path.join(result, 'dec_rescore_%s_rescore-4-0.3-0.0.csv' % s),
                                            encoding='UTF-8').read().split('\n')[:-1]]
        assert rows[0] == ['idx', 'rank', 'first_rank', 'score', 'ctc', 'att', 'lm', 'hyp', 'truth']
        items = list(ds)
        feat, lens = _mod("bin.test_asr")._pad_items(items, solver.device)
        want = solver.decoder.forward_batch(feat, lens)
        best = [r for r in rows[1:] if r[1] == '0']
        assert len(best) == len(items) > 0
        for r, d, hyps in zip(best, items, want):
            assert r[0] == d[0][0] and int(r[2]) == hyps[0].first_rank
            assert [float(v) for v in r[3:7]] == [hyps[0].score, hyps[0].ctc, hyps[0].att, hyps[0].lm]
            assert r[7] == solver.tokenizer.decode(list(hyps[0].tokens))
        out = open(os.path.join(result, 'dec_rescore_%s_output.csv' % s), encoding='UTF-8').read().splitlines()
        assert len(out) == len(items) + 1
        beam = open(os.path.join(result, 'dec_rescore_%s_beam-4-0.0.csv' % s)).read().splitlines()
        assert len(beam) == len(rows)

    # without the block: byte-identical to the unchanged code path (the parent solver of bin/test_asr.py)
    pcfg = _decode_cfg(tmp, tr_path, ckpt, 'dec_plain', **{k: v for k, v in kw.items() if k != 'vocab_candidate'})
    main.main(['--config', pcfg, '--test'] + common)
    plain = {f: open(os.path.join(result, f), 'rb').read() for f in os.listdir(result) if f.startswith('dec_plain')}
    assert sorted(plain) == ['dec_plain_%s_%s.csv' % (s, k) for s in ('dev', 'test') for k in ('beam-4-0.0', 'output')]
    test_asr = _mod("bin.test_asr")
    import argparse
    import yaml
    for f in plain:
        os.remove(os.path.join(result, f))
    config = yaml.load(open(pcfg), Loader=yaml.FullLoader)
    paras = solver.paras
    paras_plain = argparse.Namespace(**vars(paras))
    paras_plain.config = pcfg
    parent = test_asr.Solver(config, paras_plain, 'test')
    parent.load_data()
    parent.set_model()
    parent.exec()
    again = {f: open(os.path.join(result, f), 'rb').read() for f in os.listdir(result) if f.startswith('dec_plain')}
    assert again == plain
