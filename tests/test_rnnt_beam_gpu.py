"""GPU: the transducer beam search (csrc/rnnt_beam.hip, TransducerHead.beam_search).

 * the row pass against float64 on every V at which it takes another path, aligned and unaligned, with and without LM;
 * the select kernel on the tables of tests/test_rnnt_beam_cpu.py: equal to the host build bit for bit;
 * the search: one slot = the device greedy search; the cases of the CPU test = the reference's n-best lists; a batch = one
   utterance at a time; the invariant t + n_tok = iteration; the corner shapes;
 * the exhaustive setting: every finished score is -nll of ops.RNNTLoss;
 * a decode pass through the solver (tests/rnnt_beam_worker.py).

Tolerance rule of every number compared here: E = the error of the existing device path (ops.log_softmax gathered and
summed in float64 along the reference's path; ops.RNNTLoss in the exhaustive setting) against float64 on the same f32
inputs; the new path must be within 2 * max(E, floor), floor = path length * 2^-23 * max |lp| along the path."""
import importlib
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ngram_reference as NR
import rnnt_beam_reference as BR
import rnnt_reference as RR
from conftest import PKG_NAME
from test_rnnt_beam_cpu import STATE_KEYS, host_select, rbh   # noqa: F401  (rbh: the host build, a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -23
MS, ML = RR.GREEDY_MAX_SYMBOLS, RR.GREEDY_MAX_LEN


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


# ---- row pass --------------------------------------------------------------------------------------------------------------
ROWS_B, ROWS_W = 3, 4
ROWS_LIVE = (4, 2, 0)
ROW_GAP = 1e-4


def _rows_inputs(V, seed):
    """logits on a jittered grid over +-80 (neighbouring values at least 40 / V apart) with some -inf, and LM
    log-probabilities; float32"""
    rng = np.random.RandomState(seed)
    M = ROWS_B * ROWS_W
    step = 160.0 / V
    z = np.stack([(rng.permutation(V) - (V - 1) / 2.0) * step for _ in range(M)]) + (rng.rand(M, V) - 0.5) * 0.5 * step
    z = np.clip(z, -80, 80).astype(np.float32)
    z[rng.rand(M, V) < 0.05] = -np.inf
    if V <= 3:
        z[0] = np.linspace(1.0, 0.0, V)              # no -inf in row 0; row 1: every label -inf
        z[1, 1:] = -np.inf
        z[1, 0] = 0.5
    lm = rng.randn(M, V) * 2
    lm = (lm - np.log(np.exp(lm).sum(1, keepdims=True))).astype(np.float32)
    return z, lm


def _rows_reference(z, lm, lw, K):
    """float64: lse, lpb, labels [M, K] (-1 padded), values, and which rows have every rank gap >= ROW_GAP"""
    M, V = z.shape
    z64 = z.astype(np.float64)
    mx = z64.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(z64 - mx).sum(1, keepdims=True)))[:, 0]
    lp = z64 - lse[:, None]
    fused = lp + (lw * lm.astype(np.float64) if lm is not None else 0.0)
    lab = np.full((M, K), -1, np.int64)
    val = np.full((M, K), -np.inf)
    lpl = np.full((M, K), -np.inf)
    clear = np.ones((M,), bool)
    for r in range(M):
        cand = [k for k in range(1, V) if fused[r, k] > -np.inf]
        cand.sort(key=lambda k: (-fused[r, k], k))
        n = min(K, len(cand))
        lab[r, :n] = cand[:n]
        val[r, :n] = fused[r, cand[:n]]
        lpl[r, :n] = lp[r, cand[:n]]
        for j in range(min(K, len(cand) - 1)):
            if fused[r, cand[j]] - fused[r, cand[j + 1]] < ROW_GAP:
                clear[r] = False
    return lse, lp[:, 0], lab, val, clear


def _strided(a, aligned):
    """the [M, V] array on the device: 16-byte aligned base and stride, or base and stride off by one float"""
    M, V = a.shape
    ld = (V + 3) // 4 * 4 if aligned else (V + 3) // 4 * 4 + 1
    off = 0 if aligned else 1
    buf = torch.full((M * ld + 4,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[off:off + M * ld].view(M, ld)[:, :V]
    view.copy_(torch.from_numpy(a))
    assert (view.data_ptr() % 16 == 0) == aligned
    return view


def _row_pass_case(ops, V, Ks):
    live = (np.arange(ROWS_W)[None, :] < np.array(ROWS_LIVE)[:, None]).reshape(-1)
    n_live = torch.tensor(ROWS_LIVE, dtype=torch.int32, device=DEV)
    z, lm = _rows_inputs(V, 100 + V)
    ls = ops.log_softmax(torch.from_numpy(z).to(DEV)).cpu().numpy().astype(np.float64)   # the existing device path
    zd = z.copy()
    lmd = lm.copy()
    zd[~live] = np.nan                               # dead rows lie over NaN; what is checked is their padded output
    lmd[~live] = np.nan
    left_out = total = 0
    for K, aligned, with_lm in itertools.product(Ks, (True, False), (False, True)):
        lw = 0.3 if with_lm else 0.0
        lse64, lpb64, lab64, val64, clear = _rows_reference(z, lm if with_lm else None, lw, K)
        zt = _strided(zd, aligned)
        lt = _strided(lmd, aligned) if with_lm else None
        out = ops.rnnt_beam_rows(zt, ROWS_W, K, lt, lw, n_live)
        out2 = ops.rnnt_beam_rows(zt, ROWS_W, K, lt, lw, n_live)
        ops.check_errors()
        assert all(torch.equal(a, b) for a, b in zip(out, out2)), "two runs differ"
        lse, lpb, val, lab = [t.cpu().numpy() for t in out]
        # dead rows: nothing read, padded outputs
        assert (lse[~live] == 0).all() and (lpb[~live] == 0).all() and (lab[~live] == -1).all() \
            and np.isneginf(val[~live]).all()
        rows = np.nonzero(live)[0]
        ok = rows[clear[rows]]
        left_out += len(rows) - len(ok)
        total += len(rows)
        assert (lab[ok] == lab64[ok]).all(), (V, K, aligned, with_lm)
        # padded entries on every live row
        assert ((lab[rows] == -1) == (lab64[rows] == -1)).all() and np.isneginf(val[rows][lab[rows] == -1]).all()

        def check(what, got, exist, want):
            fin = np.isfinite(want)
            assert (np.isfinite(got) == fin).all() and (got[~fin] == want[~fin]).all(), what
            if not fin.any():
                return
            E = float(np.abs(exist[fin] - want[fin]).max())
            floor = EPS * float(np.abs(want[fin]).max())
            err = float(np.abs(got[fin].astype(np.float64) - want[fin]).max())
            print("rows V", V, "K", K, "aligned", aligned, "lm", with_lm, what, "E %.3g floor %.3g err %.3g" % (E, floor, err))
            assert err <= 2 * max(E, floor), (what, V, K, aligned, with_lm, err, E, floor)
        am = z[rows].argmax(1)
        exist_lse = z[rows, am].astype(np.float64) - ls[rows, am]
        check("lse", lse[rows], exist_lse, lse64[rows])
        check("lpb", lpb[rows], ls[rows, 0], lpb64[rows])
        if len(ok):
            k = np.maximum(lab64[ok], 0)
            exist_val = np.take_along_axis(ls[ok], k, 1) + (lw * np.take_along_axis(lm[ok].astype(np.float64), k, 1)
                                                              if with_lm else 0.0)
            exist_val[lab64[ok] < 0] = -np.inf
            check("val", val[ok], exist_val, val64[ok])
    # the rows left out: those whose float64 ranking has two neighbours closer than 1e-4
    print("rows V", V, "left out", left_out, "of", total)
    assert left_out <= 0.05 * total, (left_out, total)


@pytest.mark.parametrize("V", [2, 3, 63, 64, 65, 2047, 2048, 2049, 4099])
def test_row_pass_against_float64(ops, V):
    _row_pass_case(ops, V, sorted({1, min(4, V - 1), min(32, V - 1)}))


@pytest.mark.parametrize("V", [16381, 16384])
def test_row_pass_with_every_register_group(ops, V):
    """the workgroup form up to its limit: all 16 groups of 16 bytes per thread hold values (V = 16384 exactly, and a
    ragged last group); one more value is ASRK_ESHAPE"""
    _row_pass_case(ops, V, [1, 32])
    z = torch.zeros((4, 16385), dtype=torch.float32, device=DEV)
    with pytest.raises(Exception, match="shape"):
        ops.rnnt_beam_rows(z, 4, 4)


# ---- select kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 3, 8, 32])
def test_select_kernel_equals_the_host_build(ops, rbh, W):   # noqa: F811
    for seed in range(6):
        tb = BR.random_tables(W, seed)
        dv = {k: torch.from_numpy(tb[k].copy()).to(DEV) for k in STATE_KEYS + ("lpb", "val", "lab", "enc_len")}
        st = ops.RNNTBeamState(tb["B"], W, tb["K"], tb["max_len"], *[dv[k] for k in STATE_KEYS], None,
                               dv["lpb"].view(-1), dv["val"].view(-1, tb["K"]), dv["lab"].view(-1, tb["K"]))
        ops.rnnt_beam_select(st, dv["enc_len"], tb["T"], tb["max_symbols"], 0)
        ops.check_errors()
        assert host_select(rbh, tb) == 0
        for k in STATE_KEYS:                         # both started from the same arrays: every byte is the same
            assert dv[k].cpu().numpy().tobytes() == tb[k].tobytes(), (W, seed, k)


# ---- the search ---------------------------------------------------------------------------------------------------------------
def _lists(out, b):
    tokens, n_tok, score, n_hyp = out
    return [(tuple(tokens[b, h, :int(n_tok[b, h])].tolist()), float(score[b, h])) for h in range(int(n_hyp[b]))]


@pytest.mark.parametrize("module,layer,seed,bias", RR.GREEDY_CASES)
def test_one_slot_is_the_device_greedy_search(ops, module, layer, seed, bias):
    tr = _mod("src.transducer")
    head, enc, lens = RR.greedy_case(tr.TransducerHead, module, layer, seed, bias)
    head = head.to(DEV).eval()
    for ms, ml in ((MS, ML), (1, 2)):
        tokens, n_tok = head.greedy(enc.to(DEV), lens.to(DEV), ms, ml)
        bt, bn, bs, bh = head.beam_search(enc.to(DEV), lens.to(DEV), 1, ms, ml)
        ops.check_errors()
        assert bt.shape == (3, 1, ml) and bt.dtype == torch.int64 and bn.dtype == torch.int32 \
            and bs.dtype == torch.float64 and bh.tolist() == [1, 1, 1]
        assert torch.equal(bt[:, 0], tokens) and torch.equal(bn[:, 0], n_tok)
        assert bool(torch.isfinite(bs).all()) and bool((bs <= 0).all())


def _existing_lp(head, enc_b):
    """lp_fn of the existing device path for one utterance: the head's teacher-forced logits at (tokens, t) through
    ops.log_softmax, as float64"""
    ops = _mod("ops")
    cache = {}

    def lp_fn(tok, t):
        if tok not in cache:
            txt = torch.tensor([list(tok)], dtype=torch.int64, device=DEV).view(1, len(tok))
            with torch.no_grad():
                z = head(enc_b.unsqueeze(0), None, txt, None)            # [1, T, U+1, V]
                cache[tok] = ops.log_softmax(z[0, :, len(tok)].contiguous()).double().cpu()
        return cache[tok][t]
    return lp_fn


def _search_and_check(ops, head, ref, enc, lens, W, ms, ml, what, lm=None, lm_row=None, lw=0.0):
    """head.beam_search (nbest = W) on the device against the float64 reference of every utterance: the n-best lists in
    tokens and order, and every score within 2 * max(E, floor) - E from the same search on the existing device path's
    log-probabilities, floor = (T_b + max_len) * 2^-23 * max |lp| along the reference's path.  The reference's own
    margins are asserted first.  -> the device result"""
    B = enc.shape[0]
    want = BR.run_case(ref, enc, lens, W, ms, ml, lm_row, lw)
    assert min(BR.min_margin(t) for _, t in want) >= BR.MIN_MARGIN, what
    enc_d, lens_d = enc.to(DEV).contiguous(), lens.to(DEV)
    out = head.beam_search(enc_d, lens_d, W, ms, ml, nbest=W, lm=lm, lm_weight=lw)
    ops.check_errors()
    exist = BR.run_case(ref, enc, lens, W, ms, ml, lm_row, lw,
                        lp_fn=lambda b: _existing_lp(head, enc_d[b, :int(lens[b])].contiguous()))
    out_h = [t.cpu() for t in out]
    assert out_h[0].shape == (B, W, ml) and out_h[2].dtype == torch.float64
    for b in range(B):
        got = _lists(out_h, b)
        fin, trace = want[b]
        assert [g[0] for g in got] == [f[0] for f in fin], (what, b, got, fin)       # tokens and order
        assert [f[0] for f in exist[b][0]] == [f[0] for f in fin]
        ref_s = np.array([f[1] for f in fin])
        E = float(np.abs(np.array([f[1] for f in exist[b][0]]) - ref_s).max())
        floor = (int(lens[b]) + ml) * EPS * trace["max_lp"]
        err = float(np.abs(np.array([g[1] for g in got]) - ref_s).max())
        print("search", what, "utt", b, "E %.3g floor %.3g err %.3g" % (E, floor, err))
        assert err <= 2 * max(E, floor), (what, b, err, E, floor)
        # beyond each list: zeros / -inf
        n = len(got)
        assert bool((out_h[1][b, n:] == 0).all()) and bool(torch.isneginf(out_h[2][b, n:]).all())
    return out


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("W", BR.BEAM_WIDTHS)
@pytest.mark.parametrize("case", BR.BEAM_CASES)
def test_search_against_the_reference(ops, case, W, with_lm):
    tr, ng = _mod("src.transducer"), _mod("src.ngram")
    head, enc, lens = RR.greedy_case(tr.TransducerHead, *case)
    ref = RR.HeadRef.of(head, RR.GREEDY_ENC_DIM)
    image, lm_row = BR.planted_lm_model(ng, NR, RR.GREEDY_V, case[2])
    lw = BR.BEAM_LM_WEIGHT if with_lm else 0.0
    head = head.to(DEV).eval()
    lm = ng.NGramLM(image).to(DEV) if with_lm else None
    out = _search_and_check(ops, head, ref, enc, lens, W, MS, ML, "%s W %d lm %s" % (case, W, with_lm), lm,
                            lm_row if with_lm else None, lw)
    enc_d, lens_d = enc.to(DEV), lens.to(DEV)
    # the invariant of a live row after iteration i: t + n_tok = i + 1, and t inside the utterance
    seen = 0
    for i, st in head.beam_steps(enc_d, lens_d, W, MS, ML, lm, lw):
        if i in (0, 4, 9):
            n = 1 - (i & 1)
            nl, t, nt = st.n_live[n].cpu(), st.t_ptr[n].cpu(), st.n_tok[n].cpu()
            for b in range(3):
                k = int(nl[b])
                seen += k
                assert bool(((t[b, :k] + nt[b, :k]) == i + 1).all()), (i, b)
                assert bool((t[b, :k] < int(lens[b])).all())
    assert seen > 0
    # a batch of 3 = one utterance at a time, bit for bit; two runs: the same
    out2 = head.beam_search(enc_d, lens_d, W, MS, ML, nbest=W, lm=lm, lm_weight=lw)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))
    for b in range(3):
        one = head.beam_search(enc_d[b:b + 1, :int(lens[b])].contiguous(), lens_d[b:b + 1], W, MS, ML, nbest=W, lm=lm,
                               lm_weight=lw)
        ops.check_errors()
        for a, c in zip(out, one):
            assert torch.equal(a[b], c[0]), (b, a[b], c[0])


def test_search_corner_shapes(ops):
    """enc_len = 1 with B = 1 and nbest = W, and max_len = 0 (T' blanks, one empty hypothesis): tokens, order and scores
    under the same rule as every other search"""
    tr = _mod("src.transducer")
    head, enc, lens = RR.greedy_case(tr.TransducerHead, *BR.BEAM_CASES[0])
    ref = RR.HeadRef.of(head, RR.GREEDY_ENC_DIM)
    head = head.to(DEV).eval()
    out = _search_and_check(ops, head, ref, enc[:1, :1].contiguous(), torch.tensor([1]), 4, MS, ML, "enc_len 1")
    assert int(out[3][0]) >= 2, "one frame finishes several hypotheses"
    out = _search_and_check(ops, head, ref, enc, lens, 4, MS, 0, "max_len 0")
    assert out[0].shape == (3, 4, 0) and out[3].tolist() == [1, 1, 1] and out[1][:, 0].tolist() == [0, 0, 0]
    # padded frames beyond encode_len never matter
    noisy = enc.clone()
    for b in range(3):
        noisy[b, int(lens[b]):] = 7.0
    a = head.beam_search(enc.to(DEV), lens.to(DEV), 4, MS, ML, nbest=4)
    c = head.beam_search(noisy.to(DEV), lens.to(DEV), 4, MS, ML, nbest=4)
    ops.check_errors()
    assert all(torch.equal(x, y) for x, y in zip(a, c))


@pytest.mark.parametrize("T", [1, 3, 4])
def test_exhaustive_setting_against_the_fused_loss(ops, T):
    """V = 3, max_len = 2, max_symbols = 2, W = 8: nothing is pruned, so every finished score is ln P(sequence) - the
    negative of ops.RNNTLoss on that sequence"""
    tr = _mod("src.transducer")
    torch.manual_seed(T)
    head = tr.TransducerHead(3, 6, dict(module="LSTM", dim=5, layer=1, emb_dim=4, dropout=0), 7)
    ref = RR.HeadRef.of(head, 6)
    enc = torch.randn((T, 6), dtype=torch.float64, generator=torch.Generator().manual_seed(10 + T)).float()
    head = head.to(DEV).eval()
    out = head.beam_search(enc.unsqueeze(0).to(DEV), torch.tensor([T], device=DEV), 8, 2, 2, nbest=8)
    ops.check_errors()
    got = _lists([t.cpu() for t in out], 0)
    assert sorted(g[0] for g in got) == sorted(y for n in range(3) for y in itertools.product((1, 2), repeat=n))
    loss = ops.RNNTLoss(blank=0, reduction="none")
    E = err = floor = 0.0
    for tok, s in got:
        txt = torch.tensor([list(tok)], dtype=torch.int64).view(1, len(tok))
        z64 = ref.logits(enc.double().unsqueeze(0), txt)[0].detach()
        want = float(RR.alpha_lnp(RR.log_probs(z64), txt[0]))
        with torch.no_grad():
            z = head(enc.unsqueeze(0).to(DEV), None, txt.to(DEV), None)
            nll = loss(z, txt.to(DEV), torch.tensor([T], device=DEV), torch.tensor([len(tok)], device=DEV))
        E = max(E, abs(-float(nll.reshape(-1)[0]) - want))
        err = max(err, abs(s - want))
        # every alignment of the sequence is summed (max_symbols >= its length), so the path's log-probabilities are
        # the arcs of its lattice: blank at every cell, the next label at every cell that has one
        lpb, lpl = RR._lpb_lpl(RR.log_probs(z64), txt[0], 0)
        floor = max(floor, (T + 2) * EPS * max(float(lpb.abs().max()), float(lpl.abs().max()) if len(tok) else 0.0))
    print("exhaustive T", T, "E %.3g floor %.3g err %.3g" % (E, floor, err))
    assert err <= 2 * max(E, floor)


# ---- decode pass --------------------------------------------------------------------------------------------------------------
def test_decode_pass_with_the_beam_block(tmp_path):
    out = str(tmp_path / "rnnt_beam.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "rnnt_beam_worker.py"), out], capture_output=True, text=True,
                       env=dict(os.environ, ASRK_DETERMINISTIC="1"), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    # beam_size: 1 writes what the greedy search writes, and no beam file
    assert res["one"]["files"] == res["greedy"]["files"] == ["{}_dev_output.csv", "{}_test_output.csv"]
    assert res["one"]["texts"] == res["greedy"]["texts"]
    # beam_size: 4, nbest: 3: both files per set
    assert res["beam"]["files"] == ["{}_dev_beam-4-0.0.csv", "{}_dev_output.csv", "{}_test_beam-4-0.0.csv",
                                    "{}_test_output.csv"]
    for s in (0, 2):
        nbest, best = res["beam"]["texts"][s], res["beam"]["texts"][s + 1]
        assert nbest[0] == "idx\tbeam\tscore\thyp\ttruth" and best[0] == "idx\thyp\ttruth"
        assert len(best) == len(res["greedy"]["texts"][s // 2])
        rows = [ln.split("\t") for ln in nbest[1:]]
        for ln in best[1:]:
            idx, hyp, truth = ln.split("\t")
            mine = [r for r in rows if r[0] == idx]
            assert 1 <= len(mine) <= 3 and [r[1] for r in mine] == [str(j) for j in range(len(mine))]
            assert (mine[0][3] or " ") == hyp and mine[0][4] == truth
            scores = [float(r[2]) for r in mine]
            assert scores == sorted(scores, reverse=True) and all(v <= 0 for v in scores)
    # with the n-gram LM the pass runs and writes the same set of files under the LM weight's name
    assert res["lm"]["files"] == ["{}_dev_beam-2-0.3.csv", "{}_dev_output.csv", "{}_test_beam-2-0.3.csv",
                                  "{}_test_output.csv"]
    assert "n-gram" in res["rnnlm_error"]
