"""CPU: contextual biasing (src/bias.py, the argument checks of csrc/ctx_bias.hip) without a GPU.

 * the phrase-file parser: multipliers, comments, dropped phrases, the error for an empty list;
 * the builder against the dict-based restatement (tests/bias_reference.py) on random phrase sets with V = 12: node
   numbering, phi, goto and delta of every (node, token), bit for bit;
 * goto against a brute force over every sequence up to length 5;
 * the ten worked examples, the max-multiplier rule, scale folding, check_image, save / load;
 * the three ABI entries refuse bad arguments before any device call."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest

import bias_cases as BC
import bias_reference as BR
from conftest import PKG_NAME

CB = BC.bias_mod()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ---- parser ----------------------------------------------------------------------------------------------------------
def _encode(text):
    """a stand-in for the model's encoder: letters a.. -> 3.., `?` -> <unk>, anything else vanishes"""
    return [2 if ch == '?' else 3 + ord(ch) - ord('a') for ch in text if ch == '?' or 'a' <= ch <= 'z']


def test_parse_phrases(tmp_path):
    path = tmp_path / "phrases.txt"
    path.write_text("# a contact list\nabc\n\nbd\t2.5\n  # indented comment\nq?r\n123\ncab\t 0.5 \n", encoding="utf-8")
    phrases, dropped = CB.parse_phrases(str(path), _encode)
    assert phrases == [((3, 4, 5), 1.0), ((4, 6), 2.5), ((5, 3, 4), 0.5)]
    assert dropped == 2                                                # <unk> inside, and one that encodes to nothing
    for bad in ("abc\t0\n", "abc\t-1\n", "abc\tx\n", "abc\tnan\n", "abc\tinf\n"):
        path.write_text(bad, encoding="utf-8")
        with pytest.raises(ValueError, match="multiplier"):
            CB.parse_phrases(str(path), _encode)
    path.write_text("# nothing\n?\n\n", encoding="utf-8")
    with pytest.raises(ValueError, match="no usable phrase"):
        CB.parse_phrases(str(path), _encode)
    path.write_text("ab\n", encoding="utf-8")
    for special in (0, 1, 2):
        with pytest.raises(ValueError, match="no usable phrase"):
            CB.parse_phrases(str(path), lambda t, s=special: [3, s, 4])
    assert CB.is_bias_path("a/b.bias.npz") and not CB.is_bias_path("phrases.txt") and not CB.is_bias_path(None)


def test_tokenizer_encode_strips_the_appended_eos():
    class Tok:
        def encode(self, s):
            return [3 + ord(c) - ord('a') for c in s] + [1]
    assert CB.tokenizer_encode(Tok())("abc") == [3, 4, 5]


# ---- builder -----------------------------------------------------------------------------------------------------------
def _check_against_ref(phrases, V, weight, scale=1.0):
    image = CB.build_image(phrases, V, weight, scale)
    ref = BR.Ref(phrases, V, weight, scale)
    ids = ref.ids()
    paths = BR.image_nodes(image)
    assert len(image['phi']) == len(ids) and paths == {i: n for n, i in ids.items()}       # breadth-first numbering
    for n, s in ids.items():
        assert _bits(image['phi'][s]) == _bits(ref.phi(n)), n
        want = ref.row(n)
        got = BR.emulate_row(image, s)
        assert (_bits(got) == _bits(want)).all(), (n, got, want)
        for v in range(-1, V + 1):
            ns, a = BR.emulate_goto(image, s, v)
            g = ref.goto(n, v)
            assert ns == ids[g] and _bits(a) == _bits(ref.arrive(g)), (n, v)
        f = ref.fail(n)
        assert not n or ids[f] < s                                     # a fail link points to a smaller id
    return image, ref, ids


@pytest.mark.parametrize("seed", range(6))
def test_builder_equals_the_dict_restatement(seed):
    _check_against_ref(BC.random_phrases(seed), 12, 1.5)


def test_kernel_fixture_equals_the_dict_restatement():
    image, ref, ids = _check_against_ref(BC.kernel_phrases(37), 37, BC.KERNEL_WEIGHT)
    assert max(len(n) for n in ids) == 12 and np.diff(image['ext_off']).max() == 29
    assert np.diff(CB.build_image(BC.kernel_phrases(333), 333, 1.0)['ext_off']).max() == 300


@pytest.mark.parametrize("seed", range(3))
def test_goto_equals_the_longest_suffix_by_brute_force(seed):
    V = 8
    phrases = BC.random_phrases(seed, V=V, n=6, max_len=4)
    image = CB.build_image(phrases, V, 1.0)
    ref = BR.Ref(phrases, V, 1.0)
    ids = ref.ids()
    for L in range(1, 6):
        for seq in itertools.product(range(2, V), repeat=L):
            s = 0
            for v in seq:
                s, _ = BR.emulate_goto(image, s, v)
            assert s == ids[BR.brute_goto(ref.nodes, seq[:-1], seq[-1])], seq


def test_worked_examples():
    image = CB.build_image(BC.WORKED_PHRASES, 12, 1.0)
    ref = BR.Ref(BC.WORKED_PHRASES, 12, 1.0)
    for seq, total, residual in BC.WORKED:
        for got in (BR.emulate_walk(image, seq)[1:], ref.walk(seq)[1:]):
            assert (float(got[0]), float(got[1])) == (float(total), float(residual)), (seq, got)
    assert float(ref.walk((4, 5, 6, 7))[1]) == 4 + 2                  # overlapping completions are both counted


def test_total_telescopes_to_arrivals_minus_pending():
    """sum of the deltas = sum over the path of (arrive[s_i] - phi[s_i]) + phi[final state]: what is banked on the way
    plus what still pends, on random sequences (float64 from the definitions against the float32 walk)"""
    rng = np.random.RandomState(3)
    for seed in range(4):
        phrases = BC.random_phrases(seed)
        ref = BR.Ref(phrases, 12, 1.0)
        for _ in range(50):
            seq = [int(t) for t in rng.randint(3, 9, size=int(rng.randint(0, 12)))]
            n, banked = (), 0.0
            for v in seq:
                n = ref.goto(n, v)
                banked += ref.arrive(n) - ref.phi(n)
            end, tot, res = ref.walk(seq)
            assert end == n and abs(float(tot) - (banked + float(res))) < 1e-4, (phrases, seq)


def test_shared_edges_carry_the_largest_multiplier():
    ph = [((3, 4, 5), 1.0), ((3, 4, 6), 3.0), ((3, 7), 2.0)]
    image = CB.build_image(ph, 12, 2.0)
    ids = BR.Ref(ph, 12, 2.0).ids()
    phi = lambda n: float(image['phi'][ids[n]])
    assert phi((3,)) == 6.0 and phi((3, 4)) == 12.0                    # 2 * max(1, 3, 2), + 2 * max(1, 3)
    assert BR.emulate_walk(image, (3, 4, 5))[1] == np.float32(6 + 6 + 2)
    assert BR.emulate_walk(image, (3, 7))[1] == np.float32(6 + 4)
    assert image['n_phrases'] == 3


def test_scale_folding():
    """scale = 1 / lm_weight divides every edge in float64 before the float32 cast"""
    ph, lm_w = BC.random_phrases(1), 0.3
    image, ref, ids = _check_against_ref(ph, 12, 1.5, 1.0 / lm_w)
    base = CB.build_image(ph, 12, 1.5)
    assert np.allclose(image['phi'] * np.float32(lm_w), base['phi'], rtol=1e-6)
    e = 1.5 * ph[0][1] * (1.0 / lm_w)
    assert _bits(image['root_arrive'][ph[0][0][0]]) == _bits(ref.arrive(ph[0][0][:1])) and e > 0
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            CB.build_image(ph, 12, 1.5, bad)
        with pytest.raises(ValueError):
            CB.build_image(ph, 12, bad)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        CB.build_image([((3, 12), 1.0)], 12, 1.0)
    with pytest.raises(ValueError):
        CB.build_image([], 12, 1.0)


def _broken_images():
    good = CB.build_image(BC.WORKED_PHRASES, 12, 1.0)

    def edit(key, fn):
        img = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        img[key] = fn(img[key])
        return img

    def put(i, v):
        def f(a):
            a[i] = v
            return a
        return f
    E, N = len(good['ext_word']), len(good['phi'])
    return good, {
        "phi dtype": edit('phi', lambda a: a.astype(np.float64)),
        "phi[0] != 0": edit('phi', put(0, 1.0)),
        "phi not finite": edit('phi', put(1, np.nan)),
        "root_arrive short": edit('root_arrive', lambda a: a[:-1]),
        "root_arrive not finite": edit('root_arrive', put(3, np.inf)),
        "root_next outside": edit('root_next', put(5, N)),
        "root_next negative": edit('root_next', put(5, -1)),
        "ext_off not monotone": edit('ext_off', put(2, E + 1)),
        "ext_off end": edit('ext_off', put(N, E - 1)),
        "ext_off root has entries": edit('ext_off', put(1, 1)),
        "ext_off length": edit('ext_off', lambda a: a[:-1]),
        "ext_word outside": edit('ext_word', put(0, 12)),
        "ext_word negative": edit('ext_word', put(0, -1)),
        "ext_next outside": edit('ext_next', put(0, N)),
        "ext_arrive short": edit('ext_arrive', lambda a: a[:-1]),
        "ext_arrive not finite": edit('ext_arrive', put(0, np.nan)),
        "vocab_size": edit('vocab_size', lambda v: 11),
        "weight": edit('weight', lambda v: 0.0),
        "ph_off": edit('ph_off', put(1, 0)),
        "ph_tok outside": edit('ph_tok', put(0, 12)),
        "ph_mult": edit('ph_mult', put(0, 0.0)),
    }


def test_check_image_rejects_each_kind_of_broken_image():
    good, broken = _broken_images()
    CB.check_image(good)
    for name, img in broken.items():
        with pytest.raises(ValueError, match="bias image"):
            CB.check_image(img)
        with pytest.raises(ValueError, match="bias image"):
            CB.ContextBias(img)
    # the duplicate-word case on a node that certainly has two entries
    img = CB.build_image([((3, 4), 1.0), ((3, 5), 1.0)], 12, 1.0)
    img['ext_word'] = img['ext_word'].copy()
    img['ext_word'][1] = img['ext_word'][0]
    with pytest.raises(ValueError, match="bias image"):
        CB.check_image(img)


def test_save_load_round_trip(tmp_path):
    ph = BC.kernel_phrases(37)
    image = CB.build_image(ph, 37, 1.5, n_dropped=2)
    cb = CB.ContextBias(image)
    assert cb.state_width == 1 and cb.returns_logp and cb.rnn_type == 'BIAS'
    path = str(tmp_path / "list.bias.npz")
    cb.save(path)
    back = CB.ContextBias.from_file(path, 37)
    bi = back.image()
    for k in CB.TABLE_KEYS + CB.PHRASE_KEYS:
        assert bi[k].dtype == image[k].dtype and np.array_equal(bi[k], image[k]), k
    assert (bi['weight'], bi['scale'], bi['n_phrases'], bi['n_dropped']) == (1.5, 1.0, len(ph), 2)
    assert CB.image_phrases(bi) == [(tuple(p), m) for p, m in ph]
    msg = "\n".join(back.create_msg())
    assert "phrases = %d" % len(ph) in msg and "nodes = %d" % len(image['phi']) in msg \
        and "dropped phrases = 2" in msg and "1.50" in msg and path in msg
    with pytest.raises(ValueError, match="38"):
        CB.ContextBias.from_file(path, 38)
    # another weight / scale: rebuilt from the stored phrase list
    other = CB.ContextBias.from_file(path, 37, weight=2.0, scale=1.0 / 0.3).image()
    want = CB.build_image(ph, 37, 2.0, 1.0 / 0.3, n_dropped=2)
    assert all(np.array_equal(other[k], want[k]) for k in CB.TABLE_KEYS)
    with pytest.raises(ValueError, match="text encoder"):
        CB.ContextBias.from_file(str(tmp_path / "phrases.txt"), 37)
    (tmp_path / "phrases.txt").write_text("abc\nbd\t2\n", encoding="utf-8")
    cb2 = CB.ContextBias.from_file(str(tmp_path / "phrases.txt"), 37, weight=1.0, encode=_encode)
    assert cb2.n_phrases == 2 and cb2.weight == 1.0
    with pytest.raises(RuntimeError, match="GPU"):
        import torch
        cb2(torch.zeros((1, 1), dtype=torch.int64))


def test_biased_ngram_pairs_and_checks_vocabulary():
    NG = importlib.import_module(PKG_NAME + ".src.ngram")
    import ngram_cases as NC
    lm = NG.NGramLM(NG.build_image(2, NC.kernel_fixture(37, 2), 37))
    cb = CB.ContextBias(CB.build_image(BC.kernel_phrases(37), 37, 1.5))
    both = CB.BiasedNGram.pair(lm, cb, 0.3)
    assert both.state_width == 2 and both.returns_logp and both.vocab_size == 37
    assert both.bias.scale == 1.0 / 0.3 and both.bias.weight == 1.5
    assert CB.scorer_state_width(lm) == 1 and CB.scorer_state_width(both) == 2
    with pytest.raises(ValueError, match="tokens"):
        CB.BiasedNGram(lm, CB.ContextBias(CB.build_image(BC.WORKED_PHRASES, 12, 1.0)))


# ---- ABI argument checks: before any device call ---------------------------------------------------------------------
def test_abi_argument_errors_without_gpu():
    L = importlib.import_module(PKG_NAME + "._lib").load()
    z, f = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    g = ctypes.c_void_p(8192)
    V = 16
    img = [f] * 7                                     # phi, root_arrive, root_next, ext_off, ext_word, ext_arrive, ext_next

    def step(V=V, N=3, E=2, img=img, state=f, n_state=4, tok=f, par=z, out_state=g, out=f, ld=V, R=4):
        return L.asrk_bias_step_f32(V, N, E, *img, state, n_state, tok, par, 0, out_state, out, ld, R, z)

    ng = [2, V, 2, 1] + [f] * 8

    def fused(ng=ng, N=3, E=2, img=img, state=f, n_state=4, tok=f, par=z, out_state=g, out=f, ld=V, R=4):
        return L.asrk_ngram_bias_step_f32(*ng, N, E, *img, state, n_state, tok, par, 0, out_state, out, ld, R, z)

    def walk(V=V, N=3, E=2, img=img, tok=f, ld=8, n_tok=f, Lmax=8, H=4, state=f, total=f, residual=f):
        return L.asrk_bias_walk(V, N, E, *img, tok, ld, n_tok, Lmax, H, state, total, residual, z)

    for fn in (step, fused):
        assert fn(R=0) == 0 and fn(R=0, tok=z, out=z, out_state=z) == 0            # R == 0 is a no-op
        assert fn(R=-1) == -1 and fn(n_state=-1) == -1
        assert fn(N=0) == -1 and fn(E=-1) == -1
        for i in range(4):                                                           # a NULL table
            assert fn(img=img[:i] + [z] + img[i + 1:]) == -1, i
        for i in range(4, 7):                                                        # ext_* only when there are entries
            assert fn(img=img[:i] + [z] + img[i + 1:]) == -1, i
            assert fn(img=img[:i] + [z] + img[i + 1:], E=0, R=0) == 0, i
        assert fn(ld=V - 1) == -1
        assert fn(out_state=f, state=f) == -1                                        # state_out == state_in
        assert fn(tok=z) == -1 and fn(out=z) == -1 and fn(out_state=z) == -1
        assert fn(n_state=0) == -1                                                   # a state array of no rows
    assert step(V=0) == -1
    assert fused(ng=[0] + ng[1:]) == -1 and fused(ng=[9] + ng[1:]) == -1 and fused(ng=[2, 0] + ng[2:]) == -1
    for i in range(4, 9):                                                            # a NULL n-gram table
        assert fused(ng=ng[:i] + [z] + ng[i + 1:]) == -1, i
    assert fused(ng=ng[:3] + [0] + ng[4:9] + [z, z, z], R=0) == 0                    # a unigram model: no entries
    assert walk(H=0) == 0 and walk(H=0, tok=z, state=z) == 0
    assert walk(H=-1) == -1 and walk(Lmax=-1) == -1 and walk(ld=7) == -1 and walk(V=0) == -1 and walk(N=0) == -1
    assert walk(tok=z) == -1 and walk(n_tok=z) == -1 and walk(state=z) == -1 and walk(total=z) == -1 \
        and walk(residual=z) == -1
    for i in range(4):
        assert walk(img=img[:i] + [z] + img[i + 1:]) == -1, i


# ---- the decode block -----------------------------------------------------------------------------------------------
def test_take_bias_block():
    d = {'beam_size': 4, 'bias': {'path': 'names.txt'}}
    assert CB.take_bias_block(d) == {'path': 'names.txt', 'weight': 1.5} and d == {'beam_size': 4}
    assert CB.take_bias_block({'beam_size': 4}) is None
    assert CB.take_bias_block({'bias': {'path': 'a.bias.npz', 'weight': 2}}) == {'path': 'a.bias.npz', 'weight': 2.0}
    for bad in ('names.txt', {'weight': 1.0}, {'path': ''}, {'path': 'a', 'weight': 0}, {'path': 'a', 'weight': -1},
                {'path': 'a', 'weight': True}, {'path': 'a', 'weight': float('nan')}, {'path': 'a', 'scale': 2.0},
                {'path': 'a', 'weight': '1.5'}):
        with pytest.raises(ValueError, match="decode.bias"):
            CB.take_bias_block({'bias': bad})


def _solver_mod(monkeypatch, seen):
    mod = importlib.import_module(PKG_NAME + ".bin.decode_asr")

    def base_init(self, config, paras, mode):
        seen['decode'] = dict(config['decode'])
        self.config = config
        self.src_config = {'data': {'corpus': {'name': 'x', 'path': 'p', 'batch_size': 2}, 'audio': {}, 'text': {}},
                           'hparas': {}, 'model': {}}
        self.ckpdir = 'ckpt'
        config.setdefault('data', {'corpus': {'name': 'x'}})

    monkeypatch.setattr(mod.test_asr.BaseSolver, '__init__', base_init)
    return mod


def test_bias_block_never_reaches_the_beam_decoders(monkeypatch):
    import inspect
    seen = {}
    mod = _solver_mod(monkeypatch, seen)
    bias = {'path': 'names.txt', 'weight': 2.0}
    dcfg = {'beam_size': 4, 'min_len_ratio': 0.01, 'max_len_ratio': 0.3, 'ctc_weight': 0.3, 'bias': dict(bias)}
    for cls in (mod.Solver,):                                           # the solver of main.py --test
        s = cls({'decode': dict(dcfg, bias=dict(bias))}, None, 'test')
        assert 'bias' not in seen['decode'] and 'bias' not in s.config['decode'] and s.bias_cfg == bias
        params = set(inspect.signature(importlib.import_module(PKG_NAME + ".src.decode").BeamDecoder.__init__).parameters)
        assert set(s.config['decode']) <= params and 'bias' in params
        s = cls({'decode': {'beam_size': 4}}, None, 'test')
        assert s.bias_cfg is None and s.config['decode'] == {'beam_size': 4} and s.context_bias() is None


def test_rejected_combinations(monkeypatch):
    mod = _solver_mod(monkeypatch, {})
    bias = {'path': 'names.txt'}
    tr = {'enable': True, 'max_symbols': 2}
    ok = [{'beam_size': 4, 'bias': bias},
          {'beam_size': 4, 'ctc_weight': 1.0, 'vocab_candidate': 8, 'bias': bias},                     # CTC search, bias alone
          {'beam_size': 4, 'lm_weight': 0.3, 'lm_path': 'lm.arpa', 'bias': bias},
          {'beam_size': 4, 'lm_weight': 0.0, 'lm_path': 'rnnlm.pth', 'bias': bias},                   # an LM that is off
          {'beam_size': 1, 'transducer': dict(tr), 'bias': bias},                                     # selects the beam search
          {'beam_size': 1, 'lm_path': 'lm.ngram.npz', 'transducer': dict(tr, beam_size=4, lm_weight=0.2), 'bias': bias}]
    for d in ok:
        s = mod.Solver({'decode': {k: (dict(v) if isinstance(v, dict) else v) for k, v in d.items()}}, None, 'test')
        assert s.bias_cfg == {'path': 'names.txt', 'weight': 1.5}
        if 'transducer' in d:
            T = importlib.import_module(PKG_NAME + ".src.transducer")
            assert T.uses_beam(s.transducer)
    bad = [({'beam_size': 4, 'lm_weight': 0.3, 'lm_path': 'rnnlm.pth', 'lm_config': 'lm.yaml', 'bias': bias}, "RNN-LM"),
           ({'beam_size': 4, 'ctc_weight': 0.3, 'vocab_candidate': 8, 'rescore': {'enable': True}, 'bias': bias}, "rescore"),
           ({'beam_size': 1, 'transducer': dict(tr, align=True), 'bias': bias}, "align"),
           ({'beam_size': 1, 'bias': bias}, "greedy"),
           ({'beam_size': 4, 'bias': {'path': 'names.txt', 'weight': 0}}, "weight")]
    for d, why in bad:
        with pytest.raises(ValueError, match=why):
            mod.Solver({'decode': {k: (dict(v) if isinstance(v, dict) else v) for k, v in d.items()}}, None, 'test')
    # without the block nothing is checked and nothing changes
    s = mod.Solver({'decode': {'beam_size': 1}}, None, 'test')
    assert s.bias_cfg is None and s.greedy


def test_decoders_take_the_scorer_slot():
    """BeamDecoder / CTCBeamDecoder with `bias`: alone the weight is exactly 1, beside an n-gram the image is scaled"""
    import types
    asr = types.SimpleNamespace(vocab_size=37, enable_att=True, enable_ctc=True, ctc_weight=0.5)
    NG = importlib.import_module(PKG_NAME + ".src.ngram")
    import ngram_cases as NC
    cb = CB.ContextBias(CB.build_image(BC.kernel_phrases(37), 37, 1.5))
    C = importlib.import_module(PKG_NAME + ".src.ctc")
    dec = C.CTCBeamDecoder(asr, NC.vocab_range(37), 4, 8, device='cpu', bias=cb)
    assert dec.apply_lm and dec.lm_w == 1.0 and dec.lm is cb and "Contextual biasing" in "\n".join(dec.create_msg())
    with pytest.raises(ValueError, match="tokens"):
        C.CTCBeamDecoder(types.SimpleNamespace(vocab_size=38, enable_ctc=True), NC.vocab_range(38), 4, 8, device='cpu',
                         bias=cb)
    plain = C.CTCBeamDecoder(asr, NC.vocab_range(37), 4, 8, device='cpu')
    assert not plain.apply_lm and plain.bias is None and plain.create_msg() == [
        'Decode spec| CTC decoding \t| Beam size = 4 \t| LM weight = 0']
    # torch.nn.Module refuses a SimpleNamespace child: the joint decoder is checked through attach_bias
    holder = types.SimpleNamespace(asr=asr, apply_lm=True, lm_w=0.3, lm_path='lm.arpa',
                                   lm=NG.NGramLM(NG.build_image(2, NC.kernel_fixture(37, 2), 37)))
    CB.attach_bias(holder, cb)
    assert isinstance(holder.lm, CB.BiasedNGram) and holder.lm_w == 0.3 and holder.lm.bias.scale == 1.0 / 0.3
    holder = types.SimpleNamespace(asr=asr, apply_lm=True, lm_w=0.3, lm_path='rnn.pth', lm=torch_module())
    with pytest.raises(ValueError, match="RNN-LM"):
        CB.attach_bias(holder, cb)


def torch_module():
    import torch
    return torch.nn.Linear(2, 2)


# ---- the reference side of the GPU search tests -----------------------------------------------------------------------
def test_transducer_search_cases_are_decided_by_more_than_float32_noise():
    """tests/test_bias_decode_gpu.py compares only settings whose margins exceed rnnt_beam_reference.MIN_MARGIN: at least
    three of every four do, finished hypotheses stop inside a phrase, and taking the pending bonus back re-orders lists"""
    import rnnt_beam_reference as RB
    facts = [BC.rnnt_setting(*s) for s in BC.RNNT_SETTINGS]
    ok = [f["margin"] >= RB.MIN_MARGIN for f in facts]
    assert 4 * sum(ok) >= 3 * len(ok), [f["margin"] for f in facts]
    pending = sum(f["residual"](t) > 0 for f in facts for fin, _ in f["want"] for t, _ in fin)
    moved = sum([t for t, _ in b] != [t for t, _ in fin] for f in facts for b, (fin, _) in zip(f["banked"], f["want"]))
    assert pending >= 8 and moved >= 3, (pending, moved)


def test_planted_cases_on_the_cpu_references():
    """the posteriors make the phrase's tokens the runner-up at every position: the unbiased search misses the phrase,
    the biased one outputs it - the CTC search oracle and the transducer reference"""
    import ngram_cases as NC
    import rnnt_beam_reference as RB
    import rnnt_reference as RR
    from oracle import ctc_beam_oracle as CBO
    V = NC.SEARCH_V
    x, best = BC.planted_ctc(V)
    image = CB.build_image([(BC.PLANTED_PHRASE, 1.0)], V, CB.DEFAULT_WEIGHT)
    args = (x, NC.vocab_range(V), NC.SEARCH_BEAM, NC.SEARCH_CAND)
    assert list(CBO.prefix_beam_search(*args)[0]) == best
    assert list(CBO.prefix_beam_search(*args, lm_step=BC.f32_step(BR, image), lm_w=1.0)[0]) == list(BC.PLANTED_PHRASE)
    tr = importlib.import_module(PKG_NAME + ".src.transducer")
    head, enc, lens, best = BC.planted_rnnt_head(tr.TransducerHead)
    ref = RR.HeadRef.of(head, enc.shape[2])
    assert list(RB.run_case(ref, enc, lens, 4, 1, 4)[0][0][0][0]) == best
    rb = BR.Ref([(BC.PLANTED_PHRASE, 1.0)], 11, CB.DEFAULT_WEIGHT)
    fin = RB.run_case(ref, enc, lens, 4, 1, 4, lambda tok: rb.row(rb.state(tok)).astype(np.float64), 1.0)[0][0]
    assert fin[0][0] == BC.PLANTED_PHRASE and fin[0][1] - fin[1][1] > 1.0
