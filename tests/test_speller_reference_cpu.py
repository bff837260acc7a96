"""CPU: the float64 reference of the decoder loop (tests/speller_reference.py) against the project's oracle
(oracle/asr_oracle.py: attention_decode, pinned to the reference implementation's golden vectors by
tests/test_oracle_cpu.py), both in float64: decoder states, alignments and EVERY gradient - the encoder output (through
the oracle's own key / value projections), the embeddings and every weight.  Both sides are float64 restatements of
the same formulas in a different order of operations: 1e-10 relative per tensor (rounding is 1e-16 per operation)."""
import pytest
import torch

from oracle import asr_oracle as O
import speller_reference as R

TOL = 1e-10

CONFIGS = {
    "loc_h1_lstm": (dict(mode='loc', dim=37, num_head=1, v_proj=False, temperature=0.7, loc_kernel_size=4,
                         loc_kernel_num=3), dict(module='LSTM', dim=20, layer=1, dropout=0)),
    "loc_h1_gru": (dict(mode='loc', dim=37, num_head=1, v_proj=True, temperature=0.7, loc_kernel_size=11,
                        loc_kernel_num=2), dict(module='GRU', dim=20, layer=1, dropout=0)),
    "dot_h3_lstm2": (dict(mode='dot', dim=24, num_head=3, v_proj=True, temperature=0.9, loc_kernel_size=4,
                          loc_kernel_num=3), dict(module='LSTM', dim=20, layer=2, dropout=0)),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_loop_reference_equals_oracle_in_float64(name):
    att, dec = CONFIGS[name]
    cfg = dict(ctc_weight=0.0, attention=att, decoder=dec,
               encoder=dict(prenet='', module='LSTM', bidirection=False, dim=[12], dropout=[0], layer_norm=[False],
                            proj=[False], sample_rate=[1], sample_style='drop'))
    B, T, Dv, V, L = 3, 17, 12, 11, 4
    g = torch.Generator().manual_seed(5)
    sd = {k: v.double().requires_grad_(True) for k, v in O.make_state_dict(cfg, 5, V, seed=3, init_adadelta=False).items()
          if not k.startswith('encoder.')}
    enc = torch.randn(B, T, Dv, generator=g, dtype=torch.float64).requires_grad_(True)
    enc_len = torch.tensor([T, 9, 1])
    teacher = torch.randint(1, V, (B, L), generator=g)
    g1 = torch.randn(B, L, dec['dim'], generator=g, dtype=torch.float64)
    g2 = torch.randn(B, att['num_head'], L, T, generator=g, dtype=torch.float64)

    _, att_o, st_o = O.attention_decode(sd, att, dec, enc, enc_len, L, teacher)
    leaves = [enc] + list(sd.values())
    names = ['enc'] + list(sd)
    grads_o = torch.autograd.grad((st_o * g1).sum() + (att_o * g2).sum(), leaves, allow_unused=True)

    mem = O.DecodeMemory(sd, att, dec, enc, enc_len)            # the oracle's own key / value projections
    p = lambda n: sd.get(n)
    emb = sd['pre_embed.weight']
    upper = [sd['decoder.layers.%s_l%d' % (n, l)] for l in range(1, dec['layer'])
             for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    st_r, att_r = R.loop_reference(
        mem.key, mem.value, enc_len, emb[torch.zeros(B, dtype=torch.long)], emb[teacher],
        sd['attention.proj_q.weight'], sd['attention.proj_q.bias'], p('attention.att_layer.loc_conv.weight'),
        p('attention.att_layer.loc_proj.weight'), p('attention.att_layer.gen_energy.weight'),
        p('attention.att_layer.gen_energy.bias'), sd['decoder.layers.weight_ih_l0'], sd['decoder.layers.weight_hh_l0'],
        sd['decoder.layers.bias_ih_l0'], sd['decoder.layers.bias_hh_l0'], L, att['temperature'],
        1 if dec['module'] == 'GRU' else 0, att['num_head'], p('attention.merge_head.weight'),
        p('attention.merge_head.bias'), *upper)
    grads_r = torch.autograd.grad((st_r * g1).sum() + (att_r * g2).sum(), leaves, allow_unused=True)

    rel = lambda a, b: float((a - b).detach().abs().max()) / float(b.detach().abs().max())
    assert st_r.dtype == torch.float64 and st_r.shape == st_o.shape and att_r.shape == att_o.shape
    assert rel(st_r, st_o) < TOL and rel(att_r, att_o) < TOL
    for b in range(B):                                           # -inf masking: exactly zero beyond the utterance
        assert float(att_r.detach()[b, :, :, int(enc_len[b]):].abs().sum()) == 0.0
    used = 0
    for n, a, b in zip(names, grads_r, grads_o):
        assert (a is None) == (b is None), n
        if b is None:                                            # decoder.char_trans.*: the logits are not in the loss
            assert n.startswith('decoder.char_trans.'), n
            continue
        used += 1
        if n == 'attention.att_layer.gen_energy.bias':           # exactly 0 (softmax shift invariance): rounding noise
            assert float(a.abs().max()) < 1e-12 and float(b.abs().max()) < 1e-12
            continue
        assert float(b.abs().max()) > 1e-6, n                   # a gradient that vanishes would compare nothing
        assert rel(a, b) < TOL, (n, rel(a, b))
    assert used == len(names) - 2
