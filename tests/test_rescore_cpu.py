"""CPU: two-pass decoding without a GPU - argument validation of the two C entries, the float64 reference
(tests/rescore_reference.py) against independent formulas, the host ranking, the config refusals, the solver's
handling of the `rescore` block, and the score gaps the GPU tests rely on."""
import ctypes
import importlib
import types

import numpy as np
import pytest
import torch

import rescore_cases as RC
import rescore_reference as RR
from conftest import PKG_NAME
from helpers import CASES, load_golden, golden_state_dict
from oracle import asr_oracle as AO
from oracle import ctc_beam_oracle as CBO


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


@pytest.fixture(scope="module")
def lib():
    _mod("build").build(verbose=False)
    return _mod("_lib").load()


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def test_seq_logp_argument_errors_need_no_gpu(lib):
    z, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    f = lib.asrk_seq_logp_f32
    assert f(z, 8, p, z, 4, 8, 0, 0, p, z, z) == -1           # x NULL
    assert f(p, 8, z, z, 4, 8, 0, 0, p, z, z) == -1           # target NULL
    assert f(p, 8, p, z, 4, 8, 0, 0, z, z, z) == -1           # tok_logp NULL
    assert f(p, 7, p, z, 4, 8, 0, 0, p, z, z) == -1           # ldx < V
    assert f(p, 8, p, z, -1, 8, 0, 0, p, z, z) == -1          # negative M
    assert f(p, 8, p, z, 4, 0, 0, 0, p, z, z) == -1           # V <= 0
    assert f(p, 8, p, z, 4, 8, -1, 0, p, z, z) == -1          # negative R
    assert f(p, 8, p, z, 4, 8, 0, 2, p, z, z) == -1           # unknown flag
    assert f(p, 8, p, p, 4, 8, 1, 0, p, z, z) == -1           # seg_off without seq_logp
    assert f(p, 8, p, z, 4, 8, 1, 0, p, p, z) == -1           # seq_logp without seg_off
    assert f(z, 8, z, z, 0, 8, 0, 0, z, z, z) == 0            # M == 0: nothing to do


def test_ctc_score_rows_argument_errors_and_workspace_size(lib):
    z, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    ws = lib.asrk_ctc_score_rows_ws_bytes
    f = lib.asrk_ctc_score_rows_f32
    need = ws(5, 40, 3)
    assert need >= 5 * 40 * 7 * 4 and need % 16 == 0
    assert ws(6, 40, 3) > need and ws(5, 41, 3) > need and ws(5, 40, 4) > need      # monotone
    last = 0
    for R in (1, 2, 7, 640):
        for T in (1, 9, 400):
            assert ws(R, T, 64) > last or T == 1
            last = ws(R, T, 64)
        last = 0
    assert ws(0, 40, 3) == 0 and ws(5, 0, 3) == 0 and ws(5, 40, -1) == 0 and ws(5, 40, 1024) == 0
    ok = [p, 440, 11, 3, 40, 11, p, p, p, 3, 3, p, 5, 0, p, p, need, z]
    for pos, bad in ((0, z), (6, z), (7, z), (8, z), (11, z), (14, z), (15, z), (16, need - 1), (3, -1), (4, -1), (5, 0),
                     (10, -1), (12, -1), (13, -1), (13, 11), (1, -1), (2, -1), (9, 2), (15, ctypes.c_void_p(4100))):
        a = list(ok)
        a[pos] = bad
        assert f(*a) == -1, pos
    a = list(ok)
    a[12] = 0
    assert f(*a) == 0                                           # R == 0
    a = list(ok)
    a[10], a[9] = 1024, 1024
    assert f(*a) == -2                                          # 2 * Lmax + 1 > 2048


# ---- the reference against independent formulas ------------------------------------------------------------------------------
def test_reference_ctc_equals_the_oracle_recursion():
    rs = np.random.RandomState(0)
    for T, y in ((1, []), (1, [3]), (4, [2, 2, 5]), (3, [2, 2, 5]), (9, [1, 4, 4, 2]), (12, []), (7, [6]), (2, [1, 2, 3])):
        lp = RR.log_softmax(rs.randn(T, 7) * 2)
        with np.errstate(all='ignore'):
            want = -AO.ctc_numpy(lp[:, None, :], [y], [T], [len(y)])[0]
            got = RR.ctc_logp(lp, y)
        assert got == want or abs(got - want) <= 1e-12 * max(1.0, abs(want)), (T, y, got, want)
    assert RR.ctc_logp(RR.log_softmax(rs.randn(3, 7)), [2, 2, 5]) == -np.inf
    lp = RR.log_softmax(rs.randn(5, 7))
    assert abs(RR.ctc_logp(lp, []) - lp[:, 0].sum()) <= 1e-12       # the blank path
    assert RR.ctc_logp(np.zeros((0, 7)), []) == 0.0 and RR.ctc_logp(np.zeros((0, 7)), [1]) == -np.inf


def _nbest_and_scores(case):
    g = load_golden(case)
    cfg, D, V = CASES[case][0], CASES[case][1], CASES[case][2]
    sd = golden_state_dict(g)
    sd64 = RR.f64_state_dict(sd)
    feat, flen = RC.utterances(case, D)
    out = []
    for u in range(feat.shape[0]):
        f1, l1 = feat[u:u + 1, :int(flen[u])], flen[u:u + 1]
        with torch.no_grad():
            enc, _ = AO.encoder_forward(sd, cfg['encoder'], f1, l1)
            x = torch.log_softmax(AO.ctc_head(sd, enc)[0], -1).numpy()
        nbest = [list(y) for y in CBO.prefix_beam_search(x, RC.vocab_range(V), RC.BEAM, RC.CAND)]
        s_ctc, s_att, _ = RR.acoustic_scores(sd64, cfg, f1, l1, nbest)
        out.append((f1, l1, nbest, s_ctc, s_att))
    return sd64, cfg, out


def test_reference_attention_score_equals_summed_log_softmax_of_the_oracle_decoder():
    sd64, cfg, utts = _nbest_and_scores("las_hybrid_loc")
    f1, l1, nbest, _, s_att = utts[0]
    for r, y in enumerate(nbest):
        teacher = torch.tensor([list(y) + [1]], dtype=torch.long)
        with torch.no_grad():
            enc, enc_len = AO.encoder_forward(sd64, cfg['encoder'], f1.double(), l1)
            logits, _, _ = AO.attention_decode(sd64, cfg['attention'], cfg['decoder'], enc, enc_len, teacher.shape[1],
                                               teacher=teacher)
        want = float(torch.log_softmax(logits[0], -1).gather(1, teacher[0].unsqueeze(1)).sum())
        assert abs(s_att[r] - want) <= 1e-10 * max(1.0, abs(want))


@pytest.mark.parametrize("case", RC.E2E_CASES)
def test_reference_scores_of_the_gpu_cases_are_far_apart(case):
    """what tests/test_rescore_gpu.py relies on: every list has several hypotheses and adjacent final scores differ by
    more than MIN_GAP (100x the GPU path's tolerance has to stay below that; the GPU test asserts it)"""
    _, _, utts = _nbest_and_scores(case)
    for f1, l1, nbest, s_ctc, s_att in utts:
        assert len(nbest) == RC.BEAM and f1.shape[1] <= 60
        scores = [RR.combine(c, a, 0.0, RC.CTC_W, 0.0) for c, a in zip(s_ctc, s_att)]
        srt = [scores[i] for i in RR.rank(scores)]
        gaps = [a - b for a, b in zip(srt, srt[1:])]
        print(case, srt, min(gaps))
        assert min(gaps) > RC.MIN_GAP
    assert any(RR.rank([RR.combine(c, a, 0.0, RC.CTC_W, 0.0) for c, a in zip(u[3], u[4])]) != list(range(RC.BEAM))
               for u in utts)                                   # and rescoring changes the order somewhere


# ---- host ranking ------------------------------------------------------------------------------------------------------
def test_ranking_is_stable_puts_minus_inf_last_and_handles_one_and_empty_hypotheses():
    R = _mod("src.rescore")
    hyps = [[3], [4], [5], [6], [7]]
    ctc = np.array([-1.0, -2.0, -np.inf, -1.0, -2.0], dtype=np.float32)
    att = np.array([-3.0, -2.0, 0.0, -3.0, -2.0])
    got = R.rank_hypotheses(hyps, ctc, att, None, 0.5, 0.0)
    assert [h.first_rank for h in got] == [0, 1, 3, 4, 2]       # ties in first-pass order, -inf last
    assert got[-1].score == -np.inf and got[0].score == -2.0 and got[0].lm == 0.0
    assert [h.first_rank for h in got] == RR.rank([RR.combine(c, a, 0.0, 0.5, 0.0) for c, a in zip(ctc, att)])
    got = R.rank_hypotheses(hyps, ctc, att, None, 0.0, 0.0)     # ctc_weight 0: -inf still ranks last, no NaN
    assert got[-1].first_rank == 2 and got[-1].score == -np.inf and not any(np.isnan(h.score) for h in got)
    lm = np.array([0.0, -10.0, 0.0, 5.0, 0.0])
    got = R.rank_hypotheses(hyps, ctc, att, lm, 0.5, 0.3)
    assert got[0].first_rank == 3 and abs(got[0].score - (-2.0 + 1.5)) < 1e-15 and got[0].lm == 5.0
    one = R.rank_hypotheses([[8, 9]], [-1.5], [-2.5], None, 0.3, 0.0)
    assert len(one) == 1 and one[0].tokens == (8, 9) and one[0].outIndex == [8, 9] and one[0].first_rank == 0
    assert abs(one[0].score - (0.3 * -1.5 + 0.7 * -2.5)) < 1e-15
    empty = R.rank_hypotheses([[]], [-0.25], [-1.0], None, 0.3, 0.0)
    assert empty[0].tokens == () and empty[0].outIndex == []
    assert tuple(empty[0]) == ((), empty[0].score, -0.25, -1.0, 0.0, 0)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _asr(att=True, ctc=True, V=13):
    return types.SimpleNamespace(enable_att=att, enable_ctc=ctc, vocab_size=V)


def test_rescore_decoder_refuses_at_construction_with_the_reason():
    R = _mod("src.rescore")
    with pytest.raises(ValueError, match="attention"):
        R.RescoreDecoder(_asr(att=False), 4, 5, ctc_weight=0.3)
    with pytest.raises(ValueError, match="CTC head"):
        R.RescoreDecoder(_asr(ctc=False), 4, 5, ctc_weight=0.3)
    for w in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="ctc_weight"):
            R.RescoreDecoder(_asr(), 4, 5, ctc_weight=w)
    with pytest.raises(ValueError, match="prefix-beam"):
        R.RescoreDecoder(_asr(), 33, 8, ctc_weight=0.3)             # beam > 32
    with pytest.raises(ValueError, match="prefix-beam"):
        R.RescoreDecoder(_asr(V=3000), 32, 40, ctc_weight=0.3)      # beam * (cand + 1) > 1024


def test_decode_config_refusals():
    chk = _mod("src.rescore").check_decode_config
    on = {'enable': True}
    chk({'beam_size': 4, 'rescore': on, 'ctc_weight': 0.3})
    chk({'beam_size': 1})                                            # no block: nothing is checked
    chk({'beam_size': 1, 'rescore': {'enable': False}})
    with pytest.raises(ValueError, match="beam_size"):
        chk({'beam_size': 1, 'rescore': on})
    with pytest.raises(ValueError, match="align"):
        chk({'beam_size': 4, 'align': True, 'rescore': on})
    with pytest.raises(ValueError, match="ctc_weight"):
        chk({'beam_size': 4, 'ctc_weight': 1.0, 'rescore': on})
    with pytest.raises(ValueError, match="emb"):
        chk({'beam_size': 4, 'rescore': on}, {'enable': True, 'fuse': 0.5})
    chk({'beam_size': 4, 'rescore': on}, {'enable': True, 'fuse': 0})
    with pytest.raises(ValueError, match="unknown"):
        chk({'beam_size': 4, 'rescore': {'enable': True, 'nbest': 3}})


# ---- the solver -------------------------------------------------------------------------------------------------------
def test_rescore_block_never_reaches_the_other_decoders(monkeypatch):
    mod = _mod("bin.decode_asr")
    seen = {}

    def parent_init(self, config, paras, mode):
        seen['decode'] = dict(config['decode'])
        self.config = config

    monkeypatch.setattr(mod.test_asr.Solver, '__init__', parent_init)
    dcfg = {'beam_size': 4, 'min_len_ratio': 0.01, 'max_len_ratio': 0.3, 'ctc_weight': 0.3,
            'rescore': {'enable': True, 'workspace_mb': 64}}
    s = mod.Solver({'decode': dcfg}, None, 'test')
    assert 'rescore' not in seen['decode'] and 'rescore' not in s.config['decode']
    assert s.rescore == {'enable': True, 'workspace_mb': 64} and not s.align
    _mod("src.decode").BeamDecoder.__init__.__code__.co_varnames          # the parent calls BeamDecoder(**dcfg):
    import inspect
    params = set(inspect.signature(_mod("src.decode").BeamDecoder.__init__).parameters)
    assert set(seen['decode']) <= params                                  # every key left is one it takes
    s = mod.Solver({'decode': {'beam_size': 4, 'rescore': {'enable': False}}}, None, 'test')
    assert s.rescore is None and 'rescore' not in s.config['decode']
    s = mod.Solver({'decode': {'beam_size': 4}}, None, 'test')
    assert s.rescore is None and s.config['decode'] == {'beam_size': 4}


def test_solver_without_the_block_builds_the_decoders_it_always_built(monkeypatch):
    mod = _mod("bin.decode_asr")
    calls = []
    monkeypatch.setattr(mod.test_asr.Solver, 'set_model', lambda self: calls.append('parent'))
    built = []
    monkeypatch.setattr(mod, 'RescoreDecoder', lambda *a, **k: built.append((a, k)))
    s = object.__new__(mod.Solver)
    s.greedy, s.emb_decoder = False, None
    s.set_model()                                                       # a solver without a rescore attribute
    s.rescore, s.align = None, False
    s.set_model()
    assert calls == ['parent', 'parent'] and built == []


class _Recorder:
    def __init__(self):
        self.batches = []

    def forward_batch(self, feat, feat_len):
        R = _mod("src.rescore")
        self.batches.append([int(v) for v in feat_len.tolist()])
        return [R.rank_hypotheses([[int(feat[u, 0, 0])], [7]], [-1.0, -0.5], [-2.0, -0.25], None, 0.3, 0.0)
                for u in range(feat.shape[0])]


class _Tok:
    def decode(self, ids, ignore_repeat=False):
        return ' '.join(str(i) for i in ids)


def test_solver_writes_the_three_files_in_rescored_order(tmp_path, monkeypatch):
    monkeypatch.setenv('ASRK_DECODE_BATCH', '4')
    mod = _mod("bin.decode_asr")
    s = object.__new__(mod.Solver)
    items = []
    for i in range(6):
        feat = torch.zeros(1, 3 + i % 3, 2)
        feat[0, :, 0] = 100 + i
        items.append((['utt%d' % i], feat, torch.tensor([3 + i % 3]), torch.tensor([[5, i]])))
    s.config = {'decode': {'beam_size': 4, 'ctc_weight': 0.3}}
    s.rescore, s.align = {'enable': True}, False
    s.paras = types.SimpleNamespace(verbose=False)
    s.rank, s.world, s.dist, s.step = 0, 1, None, 0
    s.device = torch.device('cpu')
    s.greedy, s.ctc_only, s.enable_att = False, False, True
    s.decoder, s.tokenizer = _Recorder(), _Tok()
    s.dv_set, s.tt_set = items, items[:2]
    s.output_file = str(tmp_path / 'run') + '_{}_{}.csv'
    s.exec()
    assert [len(b) for b in s.decoder.batches] == [4, 2, 2]
    out = open(str(tmp_path / 'run') + '_dev_output.csv').read().splitlines()
    assert out[0] == 'idx\thyp\ttruth' and out[1:] == ['utt%d\t7\t5 %d' % (i, i) for i in range(6)]   # [7] wins
    beam = open(str(tmp_path / 'run') + '_dev_beam-4-0.0.csv').read().splitlines()
    assert beam[1:3] == ['utt0\t0\t7\t5 0', 'utt0\t1\t100\t5 0']
    sc = open(str(tmp_path / 'run') + '_dev_rescore-4-0.3-0.0.csv').read().splitlines()
    assert sc[0] == 'idx\trank\tfirst_rank\tscore\tctc\tatt\tlm\thyp\ttruth' and len(sc) == 13
    assert sc[1].split('\t') == ['utt0', '0', '1', repr(0.3 * -0.5 + 0.7 * -0.25), '-0.5', '-0.25', '0.0', '7', '5 0']
    assert sc[2].split('\t')[:3] == ['utt0', '1', '0']


def test_reference_scores_of_the_lm_cases_are_far_apart(tmp_path):
    """the LM tests of tests/test_rescore_gpu.py (las_hybrid_loc, LM_SEED, lm_weight 0.3): RNN-LM and n-gram, first pass
    without and with the LM (the CPU prefix-beam oracle fused with the float64 LM) - adjacent scores of all twelve
    lists are more than 3e-3 apart"""
    import ngram_cases as NC
    import ngram_reference as NR
    case = "las_hybrid_loc"
    g = load_golden(case)
    cfg, D, V = CASES[case][0], CASES[case][1], CASES[case][2]
    sd = golden_state_dict(g)
    sd64 = RR.f64_state_dict(sd)
    z = load_golden("lm_train")
    lcfg = dict(emb_tying=False, emb_dim=8, module='LSTM', dim=12, n_layers=2, dropout=0.0)
    lsd = {k[len("lstm.param."):]: torch.from_numpy(v.copy()).double() for k, v in z.items()
           if k.startswith("lstm.param.")}
    nstep = NR.f64_lm_step(NR.read_arpa(NC.joint_lm_arpa(tmp_path / "lm.arpa", V), V))

    def rnn_step(tok, hidden):
        h = (hidden or []) + [int(tok)]
        with torch.no_grad():
            logits = AO.lm_forward(lsd, lcfg, torch.tensor([h]))[0, -1]
        return torch.log_softmax(logits, -1).numpy(), h

    def s_lm(step, y):
        st, acc = None, 0.0
        for tok, tgt in zip([0] + list(y), list(y) + [1]):
            row, st = step(tok, st)
            acc += float(row[tgt])
        return acc

    feat, flen = RC.utterances(case, D, seed=RC.LM_SEED)
    worst = np.inf
    for u in range(feat.shape[0]):
        f1, l1 = feat[u:u + 1, :int(flen[u])], flen[u:u + 1]
        with torch.no_grad():
            enc, _ = AO.encoder_forward(sd, cfg['encoder'], f1, l1)
            x = torch.log_softmax(AO.ctc_head(sd, enc)[0], -1).numpy()
        for step in (rnn_step, nstep):
            for fused in (False, True):
                nbest = [list(y) for y in CBO.prefix_beam_search(x, RC.vocab_range(V), RC.BEAM, RC.CAND,
                                                                 lm_step=step if fused else None,
                                                                 lm_w=0.3 if fused else 0.0)]
                s_ctc, s_att, _ = RR.acoustic_scores(sd64, cfg, f1, l1, nbest)
                scores = [RR.combine(c, a, s_lm(step, y), RC.CTC_W, 0.3) for c, a, y in zip(s_ctc, s_att, nbest)]
                srt = [scores[i] for i in RR.rank(scores)]
                worst = min(worst, min(a - b for a, b in zip(srt, srt[1:])))
    print("smallest gap", worst)
    assert worst > 3e-3
