"""GPU: the transducer head with the stateless prediction network in the model, in both searches and in the solver.

 * the tiny ASR of tests/test_rnnt_model_gpu.py with `pred: {module: stateless, dim: 12, context: 2}` (and context 1):
   logits' loss, the gradient with respect to the encoder output and every head parameter's gradient, ctx.weight and
   emb.weight among them, against the float64 mirror (tests/rnnt_stateless_reference.py: StatelessHeadRef).  The rule is
   that file's: E is the error of the unfused pass on the same case (the head's logits through ops.log_softmax and the
   alpha recursion in f32 torch ops under autograd on the device), the fused path must be within 2 * max(E, floor),
   floor = K 2^-23 max|reference|, K = (T' + U) + (C + 1) + 3: the lattice steps, the C taps of the prediction network
   and the rounding of its input, the three linears.
 * forward_pruned: the total loss and the same gradients, lin_am / lin_lm included, against StatelessPrunedHeadRef (the
   simple joiner and the band loss of tests/rnnt_prune_reference.py on the mirror's predictor output), E from the f32
   composition of tests/test_rnnt_prune_model_gpu.py, K = 2 ((T' + U) + 3) + (C + 1).
 * greedy: the reference loop's tokens, two runs, one utterance at a time, the max_symbols = 1 / max_len = 2 run.
 * beam: W in {2, 4}, nbest = W, without LM and with the planted bigram at 0.3: tokens, order and scores by
   test_rnnt_beam_gpu's rule (its _search_and_check, on this head and this mirror); a batch of 3 = one at a time, bit for
   bit; beam_size = 1 = greedy; enc_len = 1 and max_len = 0.
   The reference side of every search case is asserted first (and on the CPU in tests/test_rnnt_stateless_cpu.py).
 * a checkpoint reloads strictly into a head rebuilt from the config and decodes the same; the solver trains the head and
   `main.py --test` writes both files of the beam block (tests/rnnt_stateless_worker.py)."""
import importlib
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import ngram_reference as NR
import rnnt_beam_reference as BR
import rnnt_prune_reference as PR
import rnnt_reference as RR
import rnnt_stateless_reference as SR
from conftest import PKG_NAME
from test_rnnt_beam_gpu import _lists, _search_and_check
from test_rnnt_gpu import _alpha_diag_lnp

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
D, V = 8, 11
MS, ML = RR.GREEDY_MAX_SYMBOLS, RR.GREEDY_MAX_LEN


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def _head_cfg(context, prune=None):
    head = {'enable': True, 'weight': 0.3, 'joint_dim': 16, 'pred': {'module': 'stateless', 'dim': 12, 'context': context}}
    if prune is not None:
        head['prune'] = prune
    return head


def _tiny_asr(context, seed, prune=None):
    asr = _mod("src.asr")
    torch.manual_seed(seed)
    enc = dict(prenet='', module='LSTM', bidirection=True, dim=[16, 16], dropout=[0, 0], layer_norm=[False, False],
               proj=[True, True], sample_rate=[2, 1], sample_style='drop')
    return asr.ASR(D, V, True, 1.0, enc, None, None, transducer=_head_cfg(context, prune)).to(DEV)


def _batch(seed, long=False):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn((3, 20, D), generator=g)
    feat_len = torch.tensor([20, 12, 16])
    for b in range(3):
        feat[b, int(feat_len[b]):] = 0
    if long:
        return feat, feat_len, torch.tensor([[3, 3, 7, 1, 4, 2], [5, 1, 0, 0, 0, 0], [9, 2, 1, 8, 0, 0]]), \
            torch.tensor([6, 2, 4])
    return feat, feat_len, torch.tensor([[3, 3, 7, 1], [5, 1, 0, 0], [9, 2, 1, 0]]), torch.tensor([4, 2, 3])


def _checker(tag, K):
    def check(what, got, exist, want):
        E = float((exist - want).abs().max())
        floor = K * 2.0 ** -23 * max(float(want.abs().max()), 1e-30)
        err = float((got - want).abs().max())
        print(tag, what, "E", E, "floor", floor, "err", err)
        assert err <= 2 * max(E, floor), what
    return check


def _compare(check, names, pm, new, exist, loss64, enc64, enc_len_h, B, T):
    (loss_n, denc_n, g_n), (loss_e, denc_e, g_e) = new, exist
    check("loss", torch.tensor(loss_n, dtype=torch.float64), torch.tensor(loss_e, dtype=torch.float64), loss64.detach())
    check("d enc", denc_n, denc_e, enc64.grad)
    pad = torch.ones((B, T), dtype=torch.bool)
    for b in range(B):
        pad[b, :enc_len_h[b]] = False
    assert bool((denc_n[pad] == 0).all()), "frames beyond encode_len get no gradient from the head"
    for k in names:
        assert float(pm[k].grad.abs().max()) > 0, k
        check(k, g_n[k], g_e[k], pm[k].grad)


# ---- training ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("context", [2, 1])
def test_logits_loss_and_gradients_against_the_float64_mirror(ops, context):
    model = _tiny_asr(context, 3).train()
    head = model.transducer
    feat, feat_len, txt, txt_len = _batch(4)
    with torch.no_grad():
        enc_out, enc_len = model.encoder(feat.to(DEV), feat_len.to(DEV))
    enc_len_h = [int(v) for v in enc_len.tolist()]
    assert enc_out.shape[:2] == (3, 10) and enc_len_h == [10, 6, 8]
    B, T, U = 3, enc_out.shape[1], txt.shape[1]
    txt_d, tl_d = txt.to(DEV), txt_len.to(DEV)
    names = [k for k, _ in head.named_parameters()]
    assert "ctx.weight" in names and "emb.weight" in names and not any(k.startswith("pred.") for k in names)

    def device_pass(fused):
        model.zero_grad()
        enc = enc_out.detach().clone().requires_grad_(True)
        logits = model.transducer_logits(enc, enc_len, txt_d, tl_d)
        assert logits.shape == (B, T, U + 1, V)
        if fused:
            loss = ops.RNNTLoss(blank=0)(logits, txt_d, enc_len, tl_d, consume_logits=True)
        else:
            lp = ops.log_softmax(logits.view(-1, V)).view(B, T, U + 1, V)
            nll = []
            for b in range(B):
                Tb, Ub = enc_len_h[b], int(txt_len[b])
                lpb = lp[b, :Tb, :Ub + 1, 0]
                lpl = lp[b, :Tb, :Ub].gather(2, txt_d[b, :Ub].view(1, Ub, 1).expand(Tb, Ub, 1)).squeeze(2)
                nll.append(-_alpha_diag_lnp(lpb, lpl, Tb, Ub))
            loss = torch.stack(nll).mean()
        loss.backward()
        ops.check_errors()
        grads = {k: p.grad.detach().cpu().double().clone() for k, p in head.named_parameters()}
        return float(loss.detach()), enc.grad.cpu().double(), grads

    ref = SR.StatelessHeadRef.of(head, model.encoder.out_dim)
    enc64 = enc_out.detach().cpu().double().requires_grad_(True)
    z64 = ref.logits(enc64, txt)
    # the predictor alone first: the device's output is the mirror's to a few roundings
    with torch.no_grad():
        p_dev = head._predict(txt_d).cpu().double()
        p_ref = ref.predict(txt)
    assert p_dev.shape == (B, U + 1, 12)
    assert float((p_dev - p_ref).abs().max()) <= 2 * (context + 1) * 2.0 ** -23 * float(p_ref.abs().max())
    loss64 = torch.stack([-RR.alpha_lnp(RR.log_probs(z64[b, :enc_len_h[b], :int(txt_len[b]) + 1]),
                                        txt[b, :int(txt_len[b])]) for b in range(B)]).mean()
    loss64.backward()
    pm = ref.param_map()
    assert set(pm) == set(names)
    exist = device_pass(fused=False)
    new = device_pass(fused=True)
    _compare(_checker("stateless C %d" % context, (T + U) + (context + 1) + 3), names, pm, new, exist, loss64, enc64,
             enc_len_h, B, T)


@pytest.mark.parametrize("S", [2, 3])
def test_pruned_loss_and_gradients_against_the_float64_mirror(ops, S):
    sw, context = 0.5, 2
    model = _tiny_asr(context, 3, {'enable': True, 'range': S, 'simple_weight': sw}).train()
    head = model.transducer
    feat, feat_len, txt, txt_len = _batch(4, long=True)
    with torch.no_grad():
        enc_out, enc_len = model.encoder(feat.to(DEV), feat_len.to(DEV))
        head.lin_am.weight.mul_(3.0)                    # a simple joiner with an opinion: the band moves
        head.lin_lm.weight.mul_(3.0)
    enc_len_h, txt_len_h = [int(v) for v in enc_len.tolist()], [int(v) for v in txt_len.tolist()]
    assert enc_out.shape[:2] == (3, 10) and enc_len_h == [10, 6, 8]
    B, T, U = 3, enc_out.shape[1], txt.shape[1]
    txt_d, tl_d = txt.to(DEV), txt_len.to(DEV)
    names = [k for k, _ in head.named_parameters()]
    assert "lin_am.weight" in names and "lin_lm.bias" in names and "ctx.weight" in names

    with torch.no_grad():                               # the device's band starts
        pred = head._predict(txt_d)
        am = ops.linear(enc_out, head.lin_am.weight, head.lin_am.bias)
        lm = ops.linear(pred, head.lin_lm.weight, head.lin_lm.bias)
        _, occ = ops.RNNTSimpleLossFn.apply(am, lm, txt_d, enc_len, tl_d, 0)
        s_d = ops.rnnt_prune_ranges(occ, enc_len, tl_d, S)
    s_h = s_d.cpu().numpy()

    def collect(loss, enc):
        loss.backward()
        ops.check_errors()
        return (float(loss.detach()), enc.grad.cpu().double(),
                {k: p.grad.detach().cpu().double().clone() for k, p in head.named_parameters()})

    def new_pass():
        model.zero_grad()
        enc = enc_out.detach().clone().requires_grad_(True)
        total, pruned, simple = model.transducer_loss_pruned(enc, enc_len, txt_d, tl_d)
        t, p, s = (float(v.detach()) for v in (total, pruned, simple))
        assert abs(t - (p + sw * s)) <= 1e-5 * abs(t)
        return collect(total, enc)

    def existing_pass():
        model.zero_grad()
        enc = enc_out.detach().clone().requires_grad_(True)
        pr = head._predict(txt_d)
        a = ops.linear(enc, head.lin_am.weight, head.lin_am.bias)
        l = ops.linear(pr, head.lin_lm.weight, head.lin_lm.bias)
        simple = ops.RNNTLoss(blank=0)(a[:, :, None, :] + l[:, None, :, :], txt_d, enc_len, tl_d)
        E = ops.linear(enc, head.lin_enc.weight, head.lin_enc.bias)
        P = ops.linear(pr, head.lin_pred.weight, head.lin_pred.bias)
        idx = (s_d.long().unsqueeze(2) + torch.arange(S, device=DEV)).clamp(max=U)
        H = torch.tanh(E.unsqueeze(2) + P[torch.arange(B, device=DEV).view(B, 1, 1), idx])
        z = ops.linear(H, head.lin_out.weight, head.lin_out.bias)
        lp = ops.log_softmax(z.view(-1, V)).view(B, T, S, V)
        nll = []
        for b in range(B):
            sb = [int(v) for v in s_h[b]]
            lpb, lpl = PR.band_terms(lp[b], txt[b], sb, enc_len_h[b], txt_len_h[b], S)
            nll.append(-PR.band_lnp(lpb, lpl, sb, enc_len_h[b], txt_len_h[b], S))
        return collect(torch.stack(nll).mean() + sw * simple, enc)

    ref = SR.StatelessPrunedHeadRef.of(head, model.encoder.out_dim)
    enc64 = enc_out.detach().cpu().double().requires_grad_(True)
    simple64, occ64 = ref.simple(enc64, txt, enc_len_h, txt_len_h)
    s64, margin = PR.ranges(occ64, enc_len_h, txt_len_h, S)
    decided = 0
    for b in range(B):
        PR.check_invariants(s_h[b], enc_len_h[b], txt_len_h[b], S)
        for t in range(enc_len_h[b]):
            if margin[b, t] >= PR.MIN_RANGE_MARGIN:
                decided += 1
                assert s_h[b, t] == s64[b, t], (b, t, s_h[b].tolist(), s64[b].tolist())
    print("stateless pruned S", S, "frames", sum(enc_len_h), "decided", decided, "starts", s_h.tolist())
    assert decided > 0
    loss64 = ref.pruned(enc64, txt, enc_len_h, txt_len_h, s_h, S).mean() + sw * simple64.mean()
    loss64.backward()
    pm = ref.param_map()
    assert set(pm) == set(names)
    exist = existing_pass()
    new = new_pass()
    _compare(_checker("stateless pruned S %d" % S, 2 * ((T + U) + 3) + (context + 1)), names, pm, new, exist, loss64,
             enc64, enc_len_h, B, T)


# ---- greedy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("context,seed,bias", SR.GREEDY_CASES)
def test_greedy_against_the_reference_loop(ops, context, seed, bias):
    tr = _mod("src.transducer")
    head, enc, lens = SR.head_case(tr.TransducerHead, context, seed, bias)
    ref = SR.StatelessHeadRef.of(head, RR.GREEDY_ENC_DIM)
    want = RR.check_greedy_case(ref, enc, lens)                                         # the reference side first
    head = head.to(DEV).eval()
    tokens, n_tok = head.greedy(enc.to(DEV), lens.to(DEV), MS, ML)
    ops.check_errors()
    assert tokens.shape == (3, ML) and tokens.dtype == torch.int64 and n_tok.shape == (3,)
    got = [tokens[b, :int(n_tok[b])].tolist() for b in range(3)]
    assert got == want
    assert all(bool((tokens[b, int(n_tok[b]):] == 0).all()) for b in range(3))
    tokens2, n_tok2 = head.greedy(enc.to(DEV), lens.to(DEV), MS, ML)                    # two runs: the same
    assert torch.equal(tokens, tokens2) and torch.equal(n_tok, n_tok2)
    for b in range(3):                                                                  # one at a time
        t1, n1 = head.greedy(enc[b:b + 1, :int(lens[b])].to(DEV).contiguous(), lens[b:b + 1].to(DEV), MS, ML)
        assert t1[0, :int(n1[0])].tolist() == want[b]
    # a cap of one symbol per frame and two tokens in all: never more than that
    t3, n3 = head.greedy(enc.to(DEV), lens.to(DEV), 1, 2)
    assert t3.shape == (3, 2) and all(int(n) <= 2 for n in n3.tolist())
    for b in range(3):
        ref_tokens, trace = ref.greedy(enc[b, :int(lens[b])].double(), 1, 2)
        assert min(tr_[2] for tr_ in trace) >= RR.MIN_MARGIN
        assert t3[b, :int(n3[b])].tolist() == ref_tokens
    # one slot of the beam search is the greedy search
    for ms, ml, (gt, gn) in ((MS, ML, (tokens, n_tok)), (1, 2, (t3, n3))):
        bt, bn, bs, bh = head.beam_search(enc.to(DEV), lens.to(DEV), 1, ms, ml)
        assert bh.tolist() == [1, 1, 1] and torch.equal(bt[:, 0], gt) and torch.equal(bn[:, 0], gn)
        assert bool(torch.isfinite(bs).all()) and bool((bs <= 0).all())
    ops.check_errors()


def test_asr_transducer_greedy_is_the_head_on_the_encoder(ops):
    model = _tiny_asr(2, 5).eval()
    feat, feat_len, _, _ = _batch(6)
    tokens, n_tok, enc_len = model.transducer_greedy(feat.to(DEV), feat_len.to(DEV), max_symbols=2, max_len_ratio=0.35)
    with torch.no_grad():
        enc_out, enc_len2 = model.encoder(feat.to(DEV), feat_len.to(DEV))
    max_len = math.ceil(enc_out.shape[1] * 0.35)
    t2, n2 = model.transducer.greedy(enc_out, enc_len2, 2, max_len)
    assert tokens.shape == (3, max_len) and torch.equal(tokens, t2) and torch.equal(n_tok, n2)
    assert torch.equal(enc_len.cpu(), enc_len2.cpu()) and bool((n_tok <= max_len).all())
    ops.check_errors()


# ---- beam ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("W", BR.BEAM_WIDTHS)
@pytest.mark.parametrize("case", SR.BEAM_CASES)
def test_beam_search_against_the_reference(ops, case, W, with_lm):
    tr, ng = _mod("src.transducer"), _mod("src.ngram")
    head, enc, lens = SR.head_case(tr.TransducerHead, *case)
    ref = SR.StatelessHeadRef.of(head, RR.GREEDY_ENC_DIM)
    image, lm_row = BR.planted_lm_model(ng, NR, RR.GREEDY_V, case[1])
    lw = BR.BEAM_LM_WEIGHT if with_lm else 0.0
    SR.check_beam_case(BR.run_case(ref, enc, lens, W, MS, ML, lm_row if with_lm else None, lw))   # the reference side
    head = head.to(DEV).eval()
    lm = ng.NGramLM(image).to(DEV) if with_lm else None
    out = _search_and_check(ops, head, ref, enc, lens, W, MS, ML, "stateless %s W %d lm %s" % (case, W, with_lm), lm,
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


def test_beam_search_corner_shapes(ops):
    """enc_len = 1 with B = 1 and nbest = W, and max_len = 0 (T' blanks, one empty hypothesis): tokens, order and scores
    under the same rule as every other search"""
    tr = _mod("src.transducer")
    head, enc, lens = SR.head_case(tr.TransducerHead, *SR.BEAM_CASES[0])
    ref = SR.StatelessHeadRef.of(head, RR.GREEDY_ENC_DIM)
    head = head.to(DEV).eval()
    out = _search_and_check(ops, head, ref, enc[:1, :1].contiguous(), torch.tensor([1]), 4, MS, ML, "enc_len 1")
    assert int(out[3][0]) >= 2, "one frame finishes several hypotheses"
    out = _search_and_check(ops, head, ref, enc, lens, 4, MS, 0, "max_len 0")
    assert out[0].shape == (3, 4, 0) and out[3].tolist() == [1, 1, 1] and out[1][:, 0].tolist() == [0, 0, 0]
    assert _lists([t.cpu() for t in out], 0)[0][0] == ()


# ---- checkpoint and decode pass -----------------------------------------------------------------------------------------------
def test_checkpoint_reloads_into_a_head_rebuilt_from_the_config(ops, tmp_path):
    model = _tiny_asr(2, 5).eval()
    feat, feat_len, txt, txt_len = _batch(6)

    def outputs(m):
        with torch.no_grad():
            enc_out, enc_len = m.encoder(feat.to(DEV), feat_len.to(DEV))
            z = m.transducer_logits(enc_out, enc_len, txt.to(DEV), txt_len.to(DEV))
        return m.transducer_greedy(feat.to(DEV), feat_len.to(DEV), max_symbols=2, max_len_ratio=0.35) + (z,)
    want = outputs(model)
    path = str(tmp_path / "stateless.pth")
    torch.save({'model': model.state_dict()}, path)
    keys = [k for k in model.state_dict() if k.startswith("transducer.")]
    assert "transducer.ctx.weight" in keys and not any(".pred." in k for k in keys)
    fresh = _tiny_asr(2, 77).eval()                       # other weights, the same config
    other = outputs(fresh)
    fresh.load_state_dict(torch.load(path, map_location='cpu')['model'], strict=True)
    got = outputs(fresh)
    ops.check_errors()
    assert all(torch.equal(a, b) for a, b in zip(want, got))          # tokens, counts, lengths and the logits' bits
    assert not torch.equal(want[3], other[3])
    # a checkpoint of another context does not load
    with pytest.raises(RuntimeError, match="ctx.weight"):
        _tiny_asr(3, 5).load_state_dict(torch.load(path, map_location='cpu')['model'], strict=True)


def test_solver_and_decode_pass(tmp_path):
    out = str(tmp_path / "rnnt_stateless.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "rnnt_stateless_worker.py"), out], capture_output=True,
                       text=True, env=dict(os.environ, ASRK_DETERMINISTIC="1"), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    trn = res["train"]
    assert len(trn["rnnt_logs"]) >= 2 and all(math.isfinite(v) and v > 0 for v in trn["rnnt_logs"])
    assert "transducer.ctx.weight" in trn["head_keys"] and not any(".pred." in k for k in trn["head_keys"])
    assert trn["head_moved"] and trn["params_finite"] and all(math.isfinite(v) for v in trn["grad_norm"])
    assert any("stateless" in m for m in trn["msgs"]) and "best_rnnt.pth" in trn["ckpts"]
    assert trn["dv_rnnt"] and all(0 <= v < 50 for v in trn["dv_rnnt"])
    dec = res["decode"]
    assert dec["files"] == ["{}_dev_beam-4-0.0.csv", "{}_dev_output.csv", "{}_test_beam-4-0.0.csv", "{}_test_output.csv"]
    for s in (0, 2):
        nbest, best = dec["texts"][s], dec["texts"][s + 1]
        assert nbest[0] == "idx\tbeam\tscore\thyp\ttruth" and best[0] == "idx\thyp\ttruth" and len(best) > 1
        rows = [ln.split("\t") for ln in nbest[1:]]
        for ln in best[1:]:
            idx, hyp, truth = ln.split("\t")
            mine = [r_ for r_ in rows if r_[0] == idx]
            assert 1 <= len(mine) <= 3 and [r_[1] for r_ in mine] == [str(j) for j in range(len(mine))]
            assert (mine[0][3] or " ") == hyp and mine[0][4] == truth
            scores = [float(r_[2]) for r_ in mine]
            assert scores == sorted(scores, reverse=True) and all(v <= 0 for v in scores)
