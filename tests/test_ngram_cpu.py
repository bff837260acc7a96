"""CPU: the back-off n-gram LM (src/ngram.py, csrc/ngram.inc, tools/ngram_lm.py) without a GPU.

 * parser: specials, .gz, missing back-off columns; every malformed word raises and is named;
 * estimator and float64 reference (tests/ngram_reference.py) check each other: sum_w p(w | h) = 1;
 * completion of pruned files changes no probability;
 * the kernel's f32 arithmetic (emulate_f32) against float64 under a DERIVED bound;
 * csrc/ngram.inc built for the host (tests/native/ngram_host.cpp): states and chain sums bit-equal to emulate_f32;
 * the prefix beam search of the device algorithm's host build, fed by emulate_f32, returns the oracle's hypotheses
   with the float64 reference as its LM - on cases where the LM decides;
 * asrk_ngram_step_f32 refuses bad arguments before any device call.

`python tests/test_ngram_cpu.py --dump FILE` writes the image, 2000 walks and their expected results for the
stand-alone sanitizer build of tests/native/ngram_host.cpp (-DNGRAM_HOST_MAIN)."""
import ctypes
import gzip
import importlib
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, HERE)

import ngram_cases as NC
import ngram_reference as NR
from conftest import PKG_NAME
from oracle import ctc_beam_oracle as CBO

NG = NC.ngram_mod()
LN10 = NC.LN10

SMALL_ARPA = """
\\data\\
ngram 1=5
ngram 2=3
ngram 3=1

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-1.5 <unk> -0.25
-0.7\t3\t-0.3
-0.9\t4

\\2-grams:
-0.2\t<s> 3\t-0.1
-0.4\t3 4
-0.6\t4 </s>

\\3-grams:
-0.05\t<s> 3 4

\\end\\
"""


def _write(path, text):
    with (gzip.open(path, "wt") if str(path).endswith(".gz") else open(path, "w")) as f:
        f.write(text)
    return str(path)


# ---- parser -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lm.arpa", "lm.arpa.gz"])
def test_parser_reads_specials_gz_and_missing_backoff(tmp_path, name):
    order, grams = NG.parse_arpa(_write(tmp_path / name, SMALL_ARPA), 6)
    assert order == 3 and [len(g) for g in grams] == [5, 3, 1]
    assert grams[0][(0,)] == (-99.0 * LN10, -0.5 * LN10)
    assert grams[0][(1,)] == (-1.0 * LN10, 0.0)                       # no back-off column
    assert grams[0][(2,)] == (-1.5 * LN10, -0.25 * LN10)              # <unk>, space separated
    assert grams[1][(0, 3)] == (-0.2 * LN10, -0.1 * LN10)
    assert grams[2][(0, 3, 4)] == (-0.05 * LN10, 0.0)
    img = NG.build_image(order, grams, 6)
    assert img["uni_logp"].dtype == np.float32 and img["uni_logp"][3] == np.float32(-0.7 * LN10)
    assert img["uni_logp"][5] == np.float32(-99.0 * LN10) and img["uni_next"][5] == 0
    assert NG.is_ngram_path("a/b.arpa") and NG.is_ngram_path("b.arpa.gz") and NG.is_ngram_path("x.ngram.npz")
    assert not NG.is_ngram_path("lm.pth") and not NG.is_ngram_path("")


@pytest.mark.parametrize("bad", ["hello", "6", "123456", "0", "1", "2", "-3", "3.0"])
def test_parser_names_the_word_and_the_line(tmp_path, bad, line=11):
    text = SMALL_ARPA.replace("-0.7\t3\t-0.3", "-0.7\t%s\t-0.3" % bad)
    with pytest.raises(ValueError) as e:
        NG.parse_arpa(_write(tmp_path / "bad.arpa", text), 6)
    assert repr(bad) in str(e.value) and "line %d" % line in str(e.value)


def test_parser_names_a_bad_word_inside_a_higher_order_gram(tmp_path):
    text = SMALL_ARPA.replace("-0.4\t3 4", "-0.4\t3 four")
    with pytest.raises(ValueError) as e:
        NG.parse_arpa(_write(tmp_path / "bad.arpa", text), 6)
    assert "'four'" in str(e.value) and "line 16" in str(e.value)


# ---- estimator <-> float64 reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 4])
def test_estimated_models_are_normalised_in_the_float64_reference(tmp_path, order):
    V = 12
    sents = NC.corpus(7, V=V, lines=300)
    m = NR.read_arpa(NC.estimated_arpa(tmp_path / "wb.arpa", sents, order), V)
    assert m.order == order
    have = [w for w in range(V) if (w,) in m.prob]
    assert 0 in have and V - 1 not in have                            # <s> is listed, the unseen id is not
    seen = {()}
    for s in sents:
        seq = [0] + s + [1]
        for i in range(len(seq)):
            for k in range(1, order):
                if i - k + 1 >= 0:
                    seen.add(tuple(seq[i - k + 1:i + 1]))
    rng = np.random.RandomState(order)
    unseen = []
    while len(unseen) < 50:
        h = tuple(int(t) for t in rng.randint(0, V, size=int(rng.randint(1, 5))))
        if order == 1 or h[-(order - 1):] not in seen:
            unseen.append(h)
    for h in sorted(seen) + unseen:
        total = sum(np.exp(NR.logp(m, h, w)) for w in have)
        assert abs(total - 1.0) <= 1e-9, (h, total)


# ---- completion of pruned files --------------------------------------------------------------------------------------
def test_builder_completes_pruned_files_without_changing_a_probability(tmp_path):
    """every `b c` whose `a b c` survives is deleted from a 3-gram file; the builder puts them back.  The 1e-12 is
    between float64 tables (the pruned file's and the builder's completed ones: the image itself stores float32);
    the image is then checked to hold exactly the completed tables' n-grams, rounded once."""
    V = 12
    path = NC.estimated_arpa(tmp_path / "full.arpa", NC.corpus(3, V=V, lines=300), 3)
    order, grams = NG.parse_arpa(path, V)
    dropped = sorted({g[1:] for g in grams[2]} & set(grams[1]))
    assert len(dropped) > 20
    pruned = [dict(grams[0]), {g: v for g, v in grams[1].items() if g not in dropped}, dict(grams[2])]
    original = NR.from_tables(3, [dict(t) for t in pruned], V)
    assert NG.complete(pruned) >= len(dropped)
    assert all(g in pruned[1] and pruned[1][g][1] == 0.0 for g in dropped)
    completed = NR.from_tables(3, pruned, V)
    for n in range(4):
        for h in itertools.product(range(V), repeat=n):
            for w in range(V):
                assert abs(NR.logp(original, h, w) - NR.logp(completed, h, w)) <= 1e-12, (h, w)
    image = NG.build_image(3, [dict(t) for t in pruned], V)
    held = NR.from_image(image)
    assert set(held.prob) == set(completed.prob)
    assert all(held.prob[g] == float(np.float32(completed.prob[g])) for g in held.prob)
    ctx = NR.image_contexts(image)
    node_of = {h: s for s, h in ctx.items()}
    assert all(image["fail"][node_of[h]] == node_of[h[1:]] for h in node_of if h)


# ---- f32 against f64 -----------------------------------------------------------------------------------------------
def _fixture_models(tmp_path):
    """three models: (image, float64 Model of the same n-grams before rounding)"""
    out = []
    for order, V in ((4, 37), (2, 64)):
        grams = NC.kernel_fixture(V, order)
        image = NG.build_image(order, grams, V)                        # completes `grams` in place
        out.append((image, NR.from_tables(order, grams, V)))
    path = NC.estimated_arpa(tmp_path / "wb3.arpa", NC.corpus(5, V=12), 3)
    out.append((NG.NGramLM.from_arpa(path, 12).image(), NR.read_arpa(path, 12)))
    return out


def test_f32_rows_against_float64_under_the_derived_bound(tmp_path):
    """|emulate_f32 - float64| <= (d + 1) * 2^-23 * S for every state and word: S = sum of the |float64 terms| of the
    entry; each stored value carries one rounding (2^-24 relative), each of the at most d + 1 adds one more on partial
    sums that S bounds.  Derived, not fitted."""
    for image, m in _fixture_models(tmp_path):
        ctx = NR.image_contexts(image)
        assert len(ctx) == len(image["bo"])
        for s, h in ctx.items():
            c, _ = NR.emulate_chain(image, s)
            d = len(c) - 1
            assert d == len(h)
            prev = ctx[s][:-1] if h else ()
            node_prev = [k for k, v in ctx.items() if v == prev][0]
            ns, row = NR.emulate_f32(image, node_prev, h[-1]) if h else (0, NR.emulate_f32(image, 0, -1)[1])
            assert ns == s
            for w in range(m.V):
                t = NR.terms(m, h, w)
                S = sum(abs(x) for x in t)
                assert abs(float(row[w]) - sum(t)) <= (d + 1) * 2.0 ** -23 * S, (h, w)


# ---- host build of csrc/ngram.inc ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ngh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ngh") / "libngh.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "native", "ngram_host.cpp")])
    L = ctypes.CDLL(so)
    L.ngh_walk.restype = None
    L.ngh_walk.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 8 + [ctypes.c_int] + [ctypes.c_void_p] * 6
    return L


def _walks(n=2000):
    """the order-4 fixture and n (state, token) pairs: every node as a start, tokens without a unigram, </s>,
    top-order contexts (states of length order - 1), tokens outside the vocabulary"""
    V, order = 37, 4
    image = NG.build_image(order, NC.kernel_fixture(V, order), V)
    ctx = NR.image_contexts(image)
    rng = np.random.RandomState(4)
    top = [s for s, h in ctx.items() if len(h) == order - 1]
    assert top
    N = len(image["bo"])
    states = rng.randint(0, N, size=n).astype(np.int32)
    tokens = rng.randint(0, V, size=n).astype(np.int64)
    states[:200] = rng.choice(top, size=200)
    states[200:200 + len(top)] = top
    tokens[200:200 + len(top)] = NC.EVERY_LEVEL
    assert len(top) <= 300
    tokens[500:540] = NC.NO_UNIGRAM[0]
    tokens[540:580] = V - 1
    tokens[580:620] = 1
    tokens[620:624] = [-1, V, V + 1000, -2 ** 40]
    return image, states, tokens


def _expected(image, states, tokens):
    n = len(states)
    st, dp = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ch, sm = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.float32)
    for i in range(n):
        st[i] = NR.emulate_advance(image, int(states[i]), int(tokens[i]))
        c, B = NR.emulate_chain(image, int(st[i]))
        dp[i] = len(c) - 1
        ch[i, :len(c)], sm[i, :len(B)] = c, B
    return st, dp, ch, sm


def _image_args(image):
    p = lambda a: a.ctypes.data
    return [int(image["order"]), int(image["vocab_size"]), len(image["bo"]), len(image["word"])] + \
        [p(image[k]) for k in NG.IMAGE_KEYS]


def test_host_build_of_ngram_inc_equals_emulate_f32(ngh):
    image, states, tokens = _walks()
    n = len(states)
    st, dp = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ch, sm = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.float32)
    ngh.ngh_walk(*_image_args(image), n, states.ctypes.data, tokens.ctypes.data, st.ctypes.data, dp.ctypes.data,
                 ch.ctypes.data, sm.ctypes.data)
    w_st, w_dp, w_ch, w_sm = _expected(image, states, tokens)
    assert (st == w_st).all() and (dp == w_dp).all()
    assert set(w_dp.tolist()) == {0, 1, 2, 3}                          # every depth was reached
    for i in range(n):
        k = dp[i] + 1
        assert (ch[i, :k] == w_ch[i, :k]).all()
        assert (sm[i, :k].view(np.uint32) == w_sm[i, :k].view(np.uint32)).all()


def test_save_load_round_trips_the_image_bit_for_bit(tmp_path):
    image, _, _ = _walks()
    lm = NG.NGramLM(image)
    path = str(tmp_path / "lm.ngram.npz")
    lm.save(path)
    assert os.path.exists(path)
    back = NG.NGramLM.from_file(path, image["vocab_size"]).image()
    assert back["order"] == image["order"] and back["vocab_size"] == image["vocab_size"]
    for k in NG.IMAGE_KEYS:
        assert back[k].dtype == image[k].dtype and back[k].tobytes() == image[k].tobytes(), k
    with pytest.raises(ValueError):
        NG.NGramLM.from_file(path, image["vocab_size"] + 1)
    broken = dict(image, fail=image["fail"].copy())
    broken["fail"][-1] = len(image["bo"])                              # a link out of the image
    with pytest.raises(ValueError):
        NG.NGramLM(broken)


# ---- search level ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pbh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pbh_ng") / "libpbh.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "native", "prefix_beam_host.cpp")])
    L = ctypes.CDLL(so)
    L.pbh_new.restype = ctypes.c_void_p
    L.pbh_new.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p]
    L.pbh_frame.restype = ctypes.c_int
    L.pbh_frame.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int,
                            ctypes.c_int]
    L.pbh_get.argtypes = [ctypes.c_void_p] * 6
    L.pbh_free.argtypes = [ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def search_lm(tmp_path_factory):
    path = NC.search_lm_arpa(tmp_path_factory.mktemp("slm") / "lm.arpa")
    return NG.NGramLM.from_arpa(path, NC.SEARCH_V).image(), NR.read_arpa(path, NC.SEARCH_V)


def oracle_hyps(m, seed, lm_w):
    x = NC.search_posteriors(seed)
    return CBO.prefix_beam_search(x, NC.vocab_range(NC.SEARCH_V), NC.SEARCH_BEAM, NC.SEARCH_CAND,
                                  lm_step=NR.f64_lm_step(m) if lm_w > 0 else None, lm_w=lm_w)


def test_the_lm_decides_in_the_oracle_on_at_least_four_of_the_six_cases(search_lm):
    _, m = search_lm
    changed = [oracle_hyps(m, seed, lm_w)[0] != oracle_hyps(m, seed, 0.0)[0] for seed, lm_w in NC.SEARCH_CASES]
    assert sum(changed) >= 4, changed


@pytest.mark.parametrize("seed,lm_w", NC.SEARCH_CASES)
def test_host_prefix_beam_with_emulated_f32_lm_equals_oracle_with_float64_lm(pbh, search_lm, seed, lm_w):
    from test_prefix_beam_cpu import run_host_algorithm
    image, m = search_lm
    x = NC.search_posteriors(seed)
    got = run_host_algorithm(pbh, x, NC.SEARCH_V, NC.vocab_range(NC.SEARCH_V), NC.SEARCH_BEAM, NC.SEARCH_CAND,
                             lm_step=NR.f32_lm_step(image), lm_w=lm_w)
    assert got == oracle_hyps(m, seed, lm_w)


# ---- ABI argument checks ---------------------------------------------------------------------------------------------
def test_step_entry_checks_its_arguments_before_any_device_call():
    build = importlib.import_module(PKG_NAME + ".build")
    build.build(verbose=False)
    L = importlib.import_module(PKG_NAME + "._lib").load()
    z, f = ctypes.c_void_p(0), ctypes.c_void_p(4096)

    def call(order=3, V=40, N=5, E=7, img=(f,) * 8, state=f, n_state=4, tok=f, par=z, p64=0, out_state=None, out=f,
             ld=40, R=4):
        out_state = ctypes.c_void_p(8192) if out_state is None else out_state
        return L.asrk_ngram_step_f32(order, V, N, E, *img, state, n_state, tok, par, p64, out_state, out, ld, R, z)

    EINVAL = -1
    assert call(R=0) == 0 and call(R=0, tok=z, out=z) == 0            # zero rows: nothing to do
    # (no call below passes every check with R > 0: the pointers are fakes and nothing may be launched)
    for kw in (dict(order=0), dict(order=9), dict(V=0), dict(V=-3), dict(R=-1), dict(ld=39), dict(N=0), dict(E=-1),
               dict(n_state=-1)):
        assert call(**kw) == EINVAL, kw
        if "R" not in kw:
            assert call(**dict(kw, R=0)) == EINVAL, kw                # the image is checked even for zero rows
    for i in range(8):
        img = [f] * 8
        img[i] = z
        assert call(img=img) == EINVAL, i
    assert call(img=[f] * 5 + [z] * 3, E=0, R=0) == 0                  # a unigram model has no entry arrays
    assert call(tok=z) == EINVAL and call(out=z) == EINVAL and call(out_state=z) == EINVAL
    assert call(out_state=f) == EINVAL                                 # state_out must not be state_in


# ---- the dump for the stand-alone sanitizer build ---------------------------------------------------------------------
def dump(path):
    image, states, tokens = _walks()
    st, dp, ch, sm = _expected(image, states, tokens)
    with open(path, "wb") as f:
        f.write(np.array([image["order"], image["vocab_size"], len(image["bo"]), len(image["word"]), len(states)],
                         np.int32).tobytes())
        for a in [image[k] for k in NG.IMAGE_KEYS] + [states, tokens, st, dp, ch, sm]:
            f.write(np.ascontiguousarray(a).tobytes())


if __name__ == "__main__":
    dump(sys.argv[sys.argv.index("--dump") + 1])
