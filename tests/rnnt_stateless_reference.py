"""TEST INFRASTRUCTURE ONLY - float64 reference of the stateless prediction network of the transducer head (Ghodsi et al.
2020; csrc/rnnt_ctx.hip), written from the definition

    Y[b,u,d] = relu(sum_{j=0}^{C-1} w[d,0,j] X[b, u-(C-1)+j, d]),   positions < 0 contribute zero,

twice and independently:

 * fwd_loops / bwd_loops / step_loops   plain indexing loops in numpy
 * fwd_conv / bwd_conv                  torch.nn.functional.conv1d on the left-padded transpose, float64, with autograd

and of the head built on it:

 * StatelessHeadRef        the analogue of rnnt_reference.HeadRef (of, load, param_map, logits, greedy); its `rnn` method
                           has the call protocol of torch's recurrent modules on one label at a time (the "state" is the
                           embeddings of the last C - 1 labels), which is all rnnt_beam_reference.beam_search asks of a
                           reference head, so that function is used as it is
 * StatelessPrunedHeadRef  the same with lin_am / lin_lm; the simple joiner and the band loss are the functions of
                           rnnt_prune_reference.PrunedHeadRef, which need `predict` only

and the case tables with their seeds (chosen on the CPU: tests/test_rnnt_stateless_cpu.py asserts what they were chosen
for on the float64 reference alone)."""
import numpy as np
import torch
import torch.nn.functional as F

import rnnt_prune_reference as PR
import rnnt_reference as RR

# ---- the kernels -----------------------------------------------------------------------------------------------------------
# (B, U1, D, C): the minimum; U1 < C; a small ordinary case; D with a scalar tail; D over one 256-lane tile with the
# largest C; the real head width
KERNEL_SHAPES = [(1, 1, 1, 1), (2, 1, 5, 3), (3, 7, 4, 2), (2, 9, 67, 4), (3, 5, 260, 8), (4, 65, 512, 2)]
# per shape: the seed of exact_case (pre-activations that are exactly 0 and negative ones both occur; the one-element
# shape cannot hold both) and the seed of random_case (under 1 % of the pre-activations within NEAR_ZERO of 0)
EXACT_SEEDS = {(1, 1, 1, 1): 0, (2, 1, 5, 3): 2, (3, 7, 4, 2): 1, (2, 9, 67, 4): 0, (3, 5, 260, 8): 0, (4, 65, 512, 2): 0}
RANDOM_SEEDS = {(1, 1, 1, 1): 0, (2, 1, 5, 3): 0, (3, 7, 4, 2): 0, (2, 9, 67, 4): 0, (3, 5, 260, 8): 0, (4, 65, 512, 2): 0}
NEAR_ZERO = 1e-5


def pre_loops(X, w):
    """X [B,U1,D], w [D,1,C] -> the pre-activation A [B,U1,D] in float64, j ascending"""
    X, w = np.asarray(X, np.float64), np.asarray(w, np.float64)
    B, U1, D = X.shape
    C = w.shape[2]
    A = np.zeros((B, U1, D))
    for b in range(B):
        for u in range(U1):
            for j in range(C):
                p = u - (C - 1) + j
                if p >= 0:
                    A[b, u] += w[:, 0, j] * X[b, p]
    return A


def fwd_loops(X, w):
    return np.maximum(pre_loops(X, w), 0.0)


def bwd_loops(X, w, dY):
    """-> (dX, dw) float64; the derivative at a pre-activation of exactly 0 is 0"""
    X, w, dY = np.asarray(X, np.float64), np.asarray(w, np.float64), np.asarray(dY, np.float64)
    B, U1, D = X.shape
    C = w.shape[2]
    dYm = dY * (pre_loops(X, w) > 0)
    dX, dw = np.zeros_like(X), np.zeros_like(w)
    for b in range(B):
        for u in range(U1):
            for j in range(C):
                q = u + (C - 1) - j
                if q < U1:
                    dX[b, u] += w[:, 0, j] * dYm[b, q]
                p = u - (C - 1) + j
                if p >= 0:
                    dw[:, 0, j] += dYm[b, u] * X[b, p]
    return dX, dw


def _conv(X, w):
    C = w.shape[2]
    return F.relu(F.conv1d(F.pad(X.transpose(1, 2), (C - 1, 0)), w, groups=w.shape[0])).transpose(1, 2)


def fwd_conv(X, w):
    with torch.no_grad():
        return _conv(torch.tensor(np.array(X), dtype=torch.float64), torch.tensor(np.array(w), dtype=torch.float64)).numpy()


def bwd_conv(X, w, dY, dtype=torch.float64):
    """-> (Y, dX, dw) through torch's conv1d and autograd in `dtype` (float32: the composition that exists without the
    new kernels)"""
    X = torch.tensor(np.array(X), dtype=dtype).requires_grad_(True)
    w = torch.tensor(np.array(w), dtype=dtype).requires_grad_(True)
    Y = _conv(X, w)
    Y.backward(torch.tensor(np.array(dY), dtype=dtype))
    return Y.detach().numpy(), X.grad.numpy(), w.grad.numpy()


def step_loops(tokens, n, emb, w):
    """one row of the decode step: tokens [Lc] ints, n labels emitted -> [D] float64, the output at position n of <sos> +
    tokens; NaN everywhere when a label the row reads lies outside [0, V)"""
    emb, w = np.asarray(emb, np.float64), np.asarray(w, np.float64)
    V, D = emb.shape
    C = w.shape[2]
    n = min(max(int(n), 0), len(tokens))
    acc = np.zeros(D)
    for k in range(C - 1, -1, -1):                 # k labels back from the current one: tap j = C - 1 - k, j ascending
        if n - k < 0:
            continue
        y = 0 if n - k == 0 else int(tokens[n - 1 - k])
        if y < 0 or y >= V:
            return np.full(D, np.nan)
        acc += w[:, 0, C - 1 - k] * emb[y]
    return np.maximum(acc, 0.0)


def exact_case(shape, seed=None):
    """X, w, dY drawn from {k/8 : |k| <= 16}: every product is a multiple of 1/64 below 4 and every sum of them exact in
    f32 (dw sums at most B*U1 = 260 products: below 2^11 in units of 2^-6)"""
    B, U1, D, C = shape
    rng = np.random.RandomState(1000 + (EXACT_SEEDS[shape] if seed is None else seed))
    draw = lambda *s: (rng.randint(-16, 17, size=s) / 8.0).astype(np.float32)   # noqa: E731
    return draw(B, U1, D), draw(D, 1, C), draw(B, U1, D)


def random_case(shape, seed=None):
    B, U1, D, C = shape
    rng = np.random.RandomState(2000 + (RANDOM_SEEDS[shape] if seed is None else seed))
    return (rng.randn(B, U1, D).astype(np.float32), (rng.randn(D, 1, C) / np.sqrt(C)).astype(np.float32),
            rng.randn(B, U1, D).astype(np.float32))


def near_zero_mask(X, w):
    """elements whose float64 pre-activation lies within NEAR_ZERO of 0: the sign, and with it the backward, may differ
    between two correct f32 evaluations"""
    return np.abs(pre_loops(X, w)) <= NEAR_ZERO


def step_case(C, Lc, V=9, D=12, seed=0):
    """-> (tokens [R, Lc] labels in [1, V), n_tok [R], emb [V, D] f32, w [D,1,C] f32) with n_tok running over
    {0, 1, C-1, C, Lc} (clamped into [0, Lc]) twice"""
    rng = np.random.RandomState(3000 + seed)
    ns = [min(max(v, 0), Lc) for v in (0, 1, C - 1, C, Lc)] * 2
    tokens = rng.randint(1, V, size=(len(ns), Lc))
    return (tokens, np.array(ns, np.int32), rng.randn(V, D).astype(np.float32),
            (rng.randn(D, 1, C) / np.sqrt(C)).astype(np.float32))


# ---- the head ------------------------------------------------------------------------------------------------------------
class StatelessHeadRef(torch.nn.Module):
    """float64 mirror of a TransducerHead with pred.module = stateless on plain torch modules: embedding, a depthwise
    nn.Conv1d without bias on the left-padded sequence, ReLU, the three linears, tanh"""

    def __init__(self, vocab_size, enc_dim, dim, context, joint_dim):
        super().__init__()
        self.dim, self.context = dim, context
        self.emb = torch.nn.Embedding(vocab_size, dim)
        self.conv = torch.nn.Conv1d(dim, dim, context, groups=dim, bias=False)
        self.lin_enc = torch.nn.Linear(enc_dim, joint_dim)
        self.lin_pred = torch.nn.Linear(dim, joint_dim)
        self.lin_out = torch.nn.Linear(joint_dim, vocab_size)
        self.double()

    LINEARS = ("lin_enc", "lin_pred", "lin_out")

    def load(self, head):
        sd = {k: v.detach().cpu().double() for k, v in head.state_dict().items()}
        own = {"emb.weight": sd["emb.weight"], "conv.weight": sd["ctx.weight"]}
        for name in self.LINEARS:
            own[name + ".weight"] = sd[name + ".weight"]
            own[name + ".bias"] = sd[name + ".bias"]
        assert len(own) == len(sd), "the head has parameters the mirror does not know"
        self.load_state_dict(own, strict=True)
        return self

    def param_map(self):
        """name in the head's state_dict -> this mirror's parameter"""
        m = {"emb.weight": self.emb.weight, "ctx.weight": self.conv.weight}
        for name in self.LINEARS:
            m[name + ".weight"] = getattr(self, name).weight
            m[name + ".bias"] = getattr(self, name).bias
        return m

    @classmethod
    def of(cls, head, enc_dim):
        assert head.emb_dim == head.dim and head.layer == 1
        return cls(head.vocab_size, enc_dim, head.dim, head.context, head.joint_dim).load(head)

    def predict(self, txt):
        """txt [B, U] -> [B, U+1, dim] on <sos> = 0, then txt"""
        inp = torch.cat([txt.new_zeros((txt.shape[0], 1)), txt], dim=1)
        x = F.pad(self.emb(inp).transpose(1, 2), (self.context - 1, 0))
        return F.relu(self.conv(x)).transpose(1, 2)

    def logits(self, enc, txt):
        """enc [B, T, D] float64, txt [B, U] -> [B, T, U+1, V]"""
        h = torch.tanh(self.lin_enc(enc).unsqueeze(2) + self.lin_pred(self.predict(txt)).unsqueeze(1))
        return self.lin_out(h)

    def rnn(self, x, state=None):
        """one label at a time with the call protocol of nn.LSTM / nn.GRU: x [1, 1, dim] the label's embedding, state the
        embeddings [k, dim] of the up to C - 1 labels before it (None: none) -> (output [1, 1, dim], new state).  Plain
        sums, independent of `predict`'s convolution."""
        C = self.context
        seq = x[0] if state is None else torch.cat([state, x[0]], dim=0)          # [k + 1, dim], the current label last
        acc = torch.zeros_like(x[0, 0])
        for j in range(C):
            back = C - 1 - j
            if back < seq.shape[0]:
                acc = acc + self.conv.weight[:, 0, j] * seq[seq.shape[0] - 1 - back]
        return torch.relu(acc).view(1, 1, -1), seq[max(seq.shape[0] - (C - 1), 0):] if C > 1 else seq[:0]

    @torch.no_grad()
    def greedy(self, enc, max_symbols, max_len, blank=0):
        """one utterance enc [T, D] -> (tokens, trace) as rnnt_reference.HeadRef.greedy: trace holds per decision (frame,
        argmax, margin between the best and the second-best logit, whether it emitted, whether the max_symbols cap alone
        kept it from emitting).  The prediction-network output is recomputed from the whole label sequence (`predict`)."""
        T = enc.shape[0]
        fe = self.lin_enc(enc)
        tokens, trace = [], []
        out = self.predict(torch.zeros((1, 0), dtype=torch.int64))[0, -1]
        t = n_sym = 0
        while t < T:
            z = self.lin_out(torch.tanh(fe[t] + self.lin_pred(out)))
            top = torch.topk(z, 2)
            k = int(top.indices[0])
            emit = not (k == blank or n_sym >= max_symbols or len(tokens) >= max_len)
            capped = k != blank and n_sym >= max_symbols and len(tokens) < max_len
            trace.append((t, k, float(top.values[0] - top.values[1]), emit, capped))
            if emit:
                tokens.append(k)
                n_sym += 1
                out = self.predict(torch.tensor([tokens]))[0, -1]
            else:
                t += 1
                n_sym = 0
        return tokens, trace


class StatelessPrunedHeadRef(StatelessHeadRef):
    """the mirror of a stateless head built with the `prune:` block: lin_am and lin_lm beside the rest; the simple joiner
    and the band loss are rnnt_prune_reference.PrunedHeadRef's, evaluated on this mirror's predictor output"""
    LINEARS = StatelessHeadRef.LINEARS + ("lin_am", "lin_lm")

    def __init__(self, vocab_size, enc_dim, dim, context, joint_dim):
        super().__init__(vocab_size, enc_dim, dim, context, joint_dim)
        self.lin_am = torch.nn.Linear(enc_dim, vocab_size)
        self.lin_lm = torch.nn.Linear(dim, vocab_size)
        self.double()

    simple = PR.PrunedHeadRef.simple
    pruned = PR.PrunedHeadRef.pruned


# ---- the cases of the search comparisons -------------------------------------------------------------------------------------
# (context, seed, blank bias): seeds for which the float64 reference alone meets rnnt_reference.check_greedy_case
GREEDY_CASES = [(2, 0, 0.5), (1, 0, 0.5)]
# (context, seed, blank bias): seeds for which the float64 reference alone meets check_beam_case for both widths, without
# LM and with the planted bigram at rnnt_beam_reference.BEAM_LM_WEIGHT
BEAM_CASES = [(2, 40, 0.5)]


def head_case(head_cls, context, seed, blank_bias, prune=None):
    """-> (head on the host, enc [3, 9, 16] f32, lens): rnnt_reference.greedy_case with the stateless predictor (dim 12)"""
    torch.manual_seed(seed)
    head = head_cls(RR.GREEDY_V, RR.GREEDY_ENC_DIM, dict(module='stateless', dim=12, context=context, dropout=0), 16,
                    prune=prune)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        head.lin_out.weight.mul_(4.0)
        head.lin_enc.weight.mul_(3.0)
        head.lin_out.bias.zero_()
        head.lin_out.bias[0] = blank_bias
    enc = torch.randn((len(RR.GREEDY_LENS), max(RR.GREEDY_LENS), RR.GREEDY_ENC_DIM), generator=g)
    for b, n in enumerate(RR.GREEDY_LENS):
        enc[b, n:] = 0
    return head, enc, torch.tensor(RR.GREEDY_LENS)


def check_beam_case(runs):
    """the reference side of one beam setting (rnnt_beam_reference.run_case's result), asserted before anything is
    compared: every decision margin is at least MIN_MARGIN and at least one merge of equal label sequences happens"""
    import rnnt_beam_reference as BR
    facts = BR.case_facts(runs)
    assert facts["margin"] >= BR.MIN_MARGIN, facts["margin"]
    assert facts["merges"] > 0, "no merge of equal label sequences"
    return facts
