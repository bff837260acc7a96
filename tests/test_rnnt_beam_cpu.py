"""CPU: the transducer beam search (csrc/rnnt_beam.inc, src/transducer.py) without a GPU.

 * the float64 reference (tests/rnnt_beam_reference.py) checks itself: with one slot it is HeadRef.greedy; in a setting
   small enough to keep every sequence, each finished score is the alpha recursion's ln P of that sequence;
 * csrc/rnnt_beam.inc built for the host (tests/native/rnnt_beam_host.cpp) equals the reference's select step exactly on
   tables with planted merges, ties, -inf values, dead and capped slots; the same file as a stand-alone program runs
   whole searches under the host sanitizers;
 * the cases of the GPU search comparison meet their conditions on the reference alone;
 * the decode block's new keys, and the argument errors of the new entry points."""
import ctypes
import importlib
import itertools
import math
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import ngram_reference as NR
import rnnt_beam_reference as BR
import rnnt_reference as RR
from conftest import PKG_NAME

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_SRC = os.path.join(HERE, "native", "rnnt_beam_host.cpp")
STATE_KEYS = ("n_live", "t_ptr", "n_sym", "n_tok", "score", "tokens", "fin_n", "fin_len", "fin_score", "fin_tok",
              "parent", "last_tok", "emit", "sel", "lm_sel")


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


# ---- the reference --------------------------------------------------------------------------------------------------------
def test_reference_logaddexp():
    rnd = random.Random(3)
    for _ in range(5000):
        a = rnd.uniform(-60, 5)
        b = a - rnd.choice([0.0, rnd.uniform(0, 45), rnd.uniform(0, 1e-3)])
        want = max(a, b) + math.log1p(math.exp(-abs(a - b)))
        assert abs(BR.lae(a, b) - want) <= 4e-15 * max(1.0, abs(want)) and BR.lae(a, b) == BR.lae(b, a)
    assert BR.lae(BR.NEG, BR.NEG) == BR.NEG and BR.lae(BR.NEG, -2.5) == -2.5 and BR.lae(-1.0, -100.0) == -1.0


@pytest.mark.parametrize("module,layer,seed,bias", RR.GREEDY_CASES)
def test_one_slot_is_the_greedy_search(module, layer, seed, bias):
    tr = _mod("src.transducer")
    head, enc, lens = RR.greedy_case(tr.TransducerHead, module, layer, seed, bias)
    ref = RR.HeadRef.of(head, RR.GREEDY_ENC_DIM)
    for ms, ml in ((RR.GREEDY_MAX_SYMBOLS, RR.GREEDY_MAX_LEN), (1, 2)):
        for b in range(enc.shape[0]):
            e = enc[b, :int(lens[b])].double()
            fin, _ = BR.beam_search(ref, e, 1, ms, ml)
            assert len(fin) == 1 and list(fin[0][0]) == ref.greedy(e, ms, ml)[0]


@pytest.mark.parametrize("T", [1, 3, 4])
def test_exhaustive_setting_sums_every_alignment(T):
    """V = 3, max_len = 2, max_symbols = 2, W = 8 (K = 2): at most 7 sequences exist and nothing is pruned, so a finished
    score is ln P(sequence) of the alpha recursion and the probabilities sum to at most 1"""
    tr = _mod("src.transducer")
    torch.manual_seed(T)
    head = tr.TransducerHead(3, 6, dict(module="LSTM", dim=5, layer=1, emb_dim=4, dropout=0), 7)
    ref = RR.HeadRef.of(head, 6)
    enc = torch.randn((T, 6), dtype=torch.float64, generator=torch.Generator().manual_seed(10 + T))
    fin, trace = BR.beam_search(ref, enc, 8, 2, 2)
    assert all(s["cut_gap"] is None for s in trace["steps"]) and not any(s["fin_overflow"] for s in trace["steps"])
    want = [y for n in range(3) for y in itertools.product((1, 2), repeat=n)]
    assert sorted(f[0] for f in fin) == sorted(want)
    total = 0.0
    for tok, s in fin:
        z = ref.logits(enc.unsqueeze(0), torch.tensor([list(tok)], dtype=torch.int64).view(1, len(tok)))[0]
        lnp = float(RR.alpha_lnp(RR.log_probs(z.detach()), torch.tensor(list(tok), dtype=torch.int64)))
        assert abs(s - lnp) <= 1e-10, (tok, s, lnp)
        total += math.exp(s)
    assert total <= 1.0 + 1e-12
    assert [f[1] for f in fin] == sorted((f[1] for f in fin), reverse=True)


# ---- host build of csrc/rnnt_beam.inc ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rbh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rbh") / "librbh.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, HOST_SRC])
    L = ctypes.CDLL(so)
    L.rnntb_lae.restype = ctypes.c_double
    L.rnntb_lae.argtypes = [ctypes.c_double] * 2
    L.rnntb_select.restype = ctypes.c_int
    L.rnntb_select.argtypes = ([ctypes.c_void_p] * 4 + [ctypes.c_int] * 6 + [ctypes.c_int64, ctypes.c_int]
                               + [ctypes.c_void_p] * 15)
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_select(L, tb, cur=0):
    return L.rnntb_select(_p(tb["lpb"]), _p(tb["val"]), _p(tb["lab"]), _p(tb["enc_len"]), tb["B"], tb["T"], tb["W"],
                          tb["K"], tb["max_symbols"], tb["max_len"], tb["tokens"].shape[3], cur,
                          *[_p(tb[k]) for k in STATE_KEYS])


def test_host_logaddexp_equals_the_reference_bit_for_bit(rbh):
    rnd = random.Random(5)
    for _ in range(20000):
        a = rnd.uniform(-80, 10)
        b = a - rnd.choice([0.0, rnd.uniform(0, 45), rnd.uniform(0, 1e-6)])
        assert rbh.rnntb_lae(a, b) == BR.lae(a, b) == rbh.rnntb_lae(b, a)
    assert rbh.rnntb_lae(BR.NEG, BR.NEG) == BR.NEG and rbh.rnntb_lae(-3.0, BR.NEG) == -3.0


@pytest.mark.parametrize("W", [1, 2, 3, 8, 32])
def test_host_select_equals_the_reference(rbh, W):
    """next beam, gather indices and finished list of the host build == select_step, exactly (scores bit for bit)"""
    seen = dict(merge=0, changed=0, overflow=0, dead=0, capped=0, ties=0, neginf=0)
    for seed in range(6):
        tb = BR.random_tables(W, seed)
        ref = BR.select_tables_reference(tb)
        assert host_select(rbh, tb) == 0
        BR.check_select_output(tb, ref)
        for r in ref:
            seen["merge"] += r["info"]["n_merge"]
            seen["changed"] += bool(r["info"]["merge_changed_cut"])
            seen["overflow"] += bool(r["info"]["fin_overflow"])
            seen["capped"] += bool(r["info"]["capped"])
            seen["ties"] += r["info"]["cut_gap"] == 0.0
        seen["dead"] += int((tb["n_live"][0] < W).sum())
        seen["neginf"] += int(np.isinf(tb["lpb"]).sum())
    # what the tables were built to contain
    assert seen["overflow"] and seen["capped"] and seen["neginf"] and (W == 1 or seen["dead"])
    if W >= 2:
        assert seen["merge"] and seen["ties"] and seen["changed"], seen


def test_host_select_argument_errors(rbh):
    tb = BR.random_tables(2, 0)
    for key, bad in (("W", 0), ("W", 33), ("K", 0), ("K", 3), ("max_len", -1), ("max_symbols", -1), ("T", 0), ("B", -1)):
        t2 = dict(tb)
        t2[key] = bad
        assert host_select(rbh, t2) == -1, (key, bad)
    assert host_select(rbh, tb, cur=2) == -1


def test_host_program_under_the_sanitizers(tmp_path):
    """the stand-alone build (-DRNNT_BEAM_HOST_MAIN): whole searches on exactly sized heap buffers under
    AddressSanitizer and UBSan, in a process of its own"""
    exe = str(tmp_path / "rnnt_beam_host")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DRNNT_BEAM_HOST_MAIN", "-o", exe, HOST_SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr


# ---- the cases of the GPU comparison, on the reference alone ---------------------------------------------------------------
def case_runs(module, layer, seed, bias):
    tr = _mod("src.transducer")
    head, enc, lens = RR.greedy_case(tr.TransducerHead, module, layer, seed, bias)
    ref = RR.HeadRef.of(head, RR.GREEDY_ENC_DIM)
    _, lm_row = BR.planted_lm_model(_mod("src.ngram"), NR, RR.GREEDY_V, seed)
    facts = {}
    for W in BR.BEAM_WIDTHS:
        for with_lm in (False, True):
            runs = BR.run_case(ref, enc, lens, W, RR.GREEDY_MAX_SYMBOLS, RR.GREEDY_MAX_LEN, lm_row if with_lm else None,
                               BR.BEAM_LM_WEIGHT if with_lm else 0.0)
            facts[(W, with_lm)] = BR.case_facts(runs)
    greedy = [tuple(ref.greedy(enc[b, :int(lens[b])].double(), RR.GREEDY_MAX_SYMBOLS, RR.GREEDY_MAX_LEN)[0])
              for b in range(enc.shape[0])]
    return facts, greedy


def test_beam_cases_meet_the_reference_conditions():
    """every margin (cut, K-th label, neighbours in the finished list) is at least 1e-3 in every case; over the cases:
    merges occur and one changes a pruning decision, the max_symbols cap binds, a finished list overflows, the utterances
    finish at different iterations, the 1-best differs from greedy somewhere and the LM changes a 1-best somewhere"""
    allf, differs_greedy, differs_lm = [], False, False
    for case in BR.BEAM_CASES:
        facts, greedy = case_runs(*case)
        for (W, with_lm), f in facts.items():
            assert f["margin"] >= BR.MIN_MARGIN, (case, W, with_lm, f["margin"])
            assert len(set(f["done_at"])) == len(f["done_at"]), (case, W, with_lm, f["done_at"])
            allf.append(f)
        differs_greedy |= any(facts[(W, False)]["best"] != greedy for W in BR.BEAM_WIDTHS)
        differs_lm |= any(facts[(W, True)]["best"] != facts[(W, False)]["best"] for W in BR.BEAM_WIDTHS)
    assert sum(f["merges"] for f in allf) > 0 and any(f["merge_changed_cut"] for f in allf)
    assert any(f["capped"] for f in allf) and any(f["fin_overflow"] for f in allf)
    assert differs_greedy and differs_lm


def test_planted_lm_image_matches_its_tables():
    """the image NGramLM is built from holds the planted bigram model (float32 roundings of the float64 tables)"""
    ng = _mod("src.ngram")
    order, grams = BR.planted_lm(RR.GREEDY_V, 6)
    m = NR.from_tables(order, [dict(g) for g in grams], RR.GREEDY_V)
    img = ng.build_image(order, [dict(g) for g in grams], RR.GREEDY_V)
    m2 = NR.from_image(img)
    for h in ((0,), (0, 3), (4, 4, 1)):
        assert np.abs(NR.row(m, h) - NR.row(m2, h)).max() <= 1e-6


# ---- config handling ------------------------------------------------------------------------------------------------------
def test_decode_block_beam_keys():
    tr = _mod("src.transducer")
    base = {'enable': True, 'max_symbols': 2, 'max_len_ratio': 0.25}
    d = {'beam_size': 7, 'transducer': dict(base)}
    assert tr.take_decode_block(d) == {'max_symbols': 2, 'max_len_ratio': 0.25} and d == {'beam_size': 7}
    assert not tr.uses_beam({'max_symbols': 2, 'max_len_ratio': 0.25}) and not tr.uses_beam(None)
    d = {'lm_path': 'lm/four.arpa.gz', 'transducer': dict(base, beam_size=4, nbest=3, lm_weight=0.25)}
    opts = tr.take_decode_block(d)
    assert opts == {'max_symbols': 2, 'max_len_ratio': 0.25, 'beam_size': 4, 'nbest': 3, 'lm_weight': 0.25}
    assert d == {'lm_path': 'lm/four.arpa.gz'} and tr.uses_beam(opts)
    assert tr.take_decode_block({'transducer': dict(base, beam_size=1)}) == dict(
        max_symbols=2, max_len_ratio=0.25, beam_size=1)
    assert not tr.uses_beam({'max_symbols': 2, 'max_len_ratio': 0.25, 'beam_size': 1})
    assert tr.uses_beam({'max_symbols': 2, 'max_len_ratio': 0.25, 'lm_weight': 0.1})
    assert tr.take_decode_block({'transducer': dict(base, beam_size=32, nbest=32)})['nbest'] == 32
    for bad in (dict(beam_size=0), dict(beam_size=33), dict(beam_size=2.5), dict(beam_size='4'), dict(beam_size=True),
                dict(nbest=0), dict(nbest=2), dict(beam_size=4, nbest=5), dict(lm_weight=-0.1),
                dict(lm_weight=float('nan'))):
        with pytest.raises(ValueError):
            tr.take_decode_block({'lm_path': 'x.arpa', 'transducer': dict(base, **bad)})
    with pytest.raises(ValueError, match="unknown"):
        tr.take_decode_block({'transducer': dict(base, beam=2)})
    # a disabled block is not validated further, as before
    assert tr.take_decode_block({'transducer': {'enable': False, 'beam_size': 99}}) is None
    # LM fusion is n-gram only
    for path in ('ckpt/lm/best_ppx.pth', '', None):
        with pytest.raises(ValueError, match="n-gram"):
            tr.take_decode_block({'lm_path': path, 'transducer': dict(base, beam_size=4, lm_weight=0.3)})
    with pytest.raises(ValueError, match="n-gram"):
        tr.take_decode_block({'transducer': dict(base, lm_weight=0.3)})
    assert tr.take_decode_block({'lm_path': 'best_ppx.pth', 'transducer': dict(base, beam_size=4, lm_weight=0.0)})
    assert tr.take_decode_block({'lm_path': 'm.ngram.npz', 'transducer': dict(base, lm_weight=0.5)})['lm_weight'] == 0.5


def test_beam_search_rejects_other_language_models():
    tr = _mod("src.transducer")
    head = tr.TransducerHead(5, 4, dict(module="LSTM", dim=4, layer=1, emb_dim=4, dropout=0), 4)
    with pytest.raises(NotImplementedError, match="NGramLM"):
        head.beam_search(torch.zeros((1, 2, 4)), torch.tensor([2]), 2, 2, 3, lm=torch.nn.Linear(2, 2), lm_weight=0.3)
    for kw in (dict(beam_size=0), dict(beam_size=33), dict(beam_size=2, nbest=3)):
        with pytest.raises(ValueError):
            head.beam_search(torch.zeros((1, 2, 4)), torch.tensor([2]), kw["beam_size"], 2, 3, nbest=kw.get("nbest", 1))


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    """null pointers and impossible sizes are ASRK_EINVAL (-1) / ASRK_ESHAPE (-2) before any HIP call; B == 0 is ASRK_OK"""
    _mod("build").build(verbose=False)
    L = _mod("_lib").load()
    z, f = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    # joint: E, lde, P, ldp, t_ptr, B, T, W, J, H, ldh
    js = [f, 8, f, 8, f, 2, 3, 4, 8, f, 8, z]
    for pos, bad in ((0, z), (2, z), (4, z), (9, z), (1, 7), (3, 7), (10, 7), (5, -1), (6, 0), (7, 0), (8, 0)):
        a = list(js)
        a[pos] = bad
        assert L.asrk_rnnt_joint_slots_f32(*a) == -1, pos
    assert L.asrk_rnnt_joint_slots_f32(f, 8, f, 8, f, 2 ** 30, 3, 4, 8, f, 8, z) == -2
    assert L.asrk_rnnt_joint_slots_f32(z, 8, z, 8, z, 0, 3, 4, 8, z, 8, z) == 0
    # rows: z, ldz, lm, ldlm, lm_weight, n_live, B, W, V, K, blank, lse, lpb, val, lab
    rs = [f, 12, f, 12, 0.3, f, 2, 4, 11, 4, 0, f, f, f, f, z]
    for pos, bad in ((0, z), (11, z), (12, z), (13, z), (14, z), (1, 10), (3, 10), (6, -1), (7, 0), (7, 33), (8, 1),
                     (9, 0), (9, 11), (9, 33), (10, -1), (10, 11)):
        a = list(rs)
        a[pos] = bad
        assert L.asrk_rnnt_beam_rows_f32(*a) == -1, pos
    a = list(rs)
    a[1], a[3], a[8] = 16400, 16400, 16385           # a row no longer fits its workgroup's registers
    assert L.asrk_rnnt_beam_rows_f32(*a) == -2
    a = list(rs)
    a[2], a[3], a[5] = z, 0, z                       # no LM, every row live: fine as far as the arguments go
    a[6] = 0
    assert L.asrk_rnnt_beam_rows_f32(*a) == 0
    # select: lpb, val, lab, enc_len, B, T, W, K, max_symbols, max_len, tok_stride, cur, then 15 state / output arrays
    ss = [f, f, f, f, 2, 5, 4, 4, 2, 6, 6, 0] + [f] * 15 + [z]
    for pos in list(range(4)) + list(range(12, 27)):
        a = list(ss)
        a[pos] = z
        assert L.asrk_rnnt_beam_select(*a) == -1, pos
    for pos, bad in ((4, -1), (5, 0), (6, 0), (6, 33), (7, 0), (7, 5), (8, -1), (9, -1), (10, 5), (10, 0), (11, 2)):
        a = list(ss)
        a[pos] = bad
        assert L.asrk_rnnt_beam_select(*a) == -1, (pos, bad)
    a = list(ss)
    a[4] = 0
    assert L.asrk_rnnt_beam_select(*a) == 0
