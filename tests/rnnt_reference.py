"""float64 reference of the RNN-transducer head, written from the definitions (Graves 2012), for the rnnt tests:

 * alpha_lnp      the alpha recursion in torch ops (differentiable: autograd gives the gradient)
 * beta_lnp       an independent beta recursion
 * closed_form    the closed-form gradient of nll with respect to the logits from alpha and beta
 * batch_nll_grad both on a padded batch: nll [B] and the gradient with zeros outside every lattice
 * HeadRef        a float64 mirror of TransducerHead on plain torch modules (embedding, LSTM/GRU, three linears, tanh)
 * greedy         the greedy search, one utterance at a time, with the margin of every decision

With lp = z - logsumexp_v z, lpb(t,u) = lp[t,u,blank], lpl(t,u) = lp[t,u,y_{u+1}]:
   alpha(0,0) = 0; alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t,u-1) + lpl(t,u-1))
   beta(T-1,U) = lpb(T-1,U); beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t,u+1))
   ln P = alpha(T-1,U) + lpb(T-1,U) = beta(0,0)."""
import torch

NEG = float("-inf")


def log_probs(z):
    return z - torch.logsumexp(z, dim=-1, keepdim=True)


def _lpb_lpl(lp, y, blank):
    """lp [T, U+1, V], y [U] -> lpb [T, U+1], lpl [T, U]"""
    U = y.numel()
    lpb = lp[:, :, blank]
    lpl = lp[:, :U, :].gather(2, y.view(1, U, 1).expand(lp.shape[0], U, 1)).squeeze(2) if U else lp[:, :0, 0]
    return lpb, lpl


def alpha_lattice(lp, y, blank=0):
    """lp [T, U+1, V] log-probabilities of one utterance, y [U] -> (alpha as a nested list of 0-d tensors, ln P).
    Built from torch ops only, so autograd differentiates it in whatever dtype lp has."""
    T, U1 = lp.shape[0], lp.shape[1]
    lpb, lpl = _lpb_lpl(lp, y, blank)
    a = [[None] * U1 for _ in range(T)]
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                a[t][u] = lp.new_zeros(())
                continue
            terms = []
            if t > 0:
                terms.append(a[t - 1][u] + lpb[t - 1, u])
            if u > 0:
                terms.append(a[t][u - 1] + lpl[t, u - 1])
            a[t][u] = terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1])
    return a, a[T - 1][U1 - 1] + lpb[T - 1, U1 - 1]


def alpha_lnp(lp, y, blank=0):
    return alpha_lattice(lp, y, blank)[1]


def beta_lattice(lp, y, blank=0):
    T, U1 = lp.shape[0], lp.shape[1]
    U = U1 - 1
    lpb, lpl = _lpb_lpl(lp, y, blank)
    b = [[None] * U1 for _ in range(T)]
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            if t == T - 1 and u == U:
                b[t][u] = lpb[t, u]
                continue
            terms = []
            if t + 1 < T:
                terms.append(lpb[t, u] + b[t + 1][u])
            if u < U:
                terms.append(lpl[t, u] + b[t][u + 1])
            b[t][u] = terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1])
    return b, b[0][0]


def beta_lnp(lp, y, blank=0):
    return beta_lattice(lp, y, blank)[1]


def closed_form(z, y, blank=0):
    """d nll / d z [T, U+1, V] of one utterance from alpha and beta (no autograd):
    gamma(t,u) softmax_v - [v = blank] exp(alpha + lpb + beta(t+1,u) - lnP) - [v = y_{u+1}] exp(alpha + lpl + beta(t,u+1)
    - lnP), with beta(T,U) := 0 and every other beta outside the lattice -inf"""
    with torch.no_grad():
        lp = log_probs(z)
        T, U1, V = lp.shape
        U = U1 - 1
        a, lnp = alpha_lattice(lp, y, blank)
        b, _ = beta_lattice(lp, y, blank)
        g = torch.zeros_like(lp)
        for t in range(T):
            for u in range(U1):
                g[t, u] = torch.exp(a[t][u] + b[t][u] - lnp + lp[t, u])
                bt = b[t + 1][u] if t + 1 < T else (lp.new_zeros(()) if u == U else lp.new_tensor(NEG))
                g[t, u, blank] -= torch.exp(a[t][u] + lp[t, u, blank] + bt - lnp)
                if u < U:
                    g[t, u, y[u]] -= torch.exp(a[t][u] + lp[t, u, y[u]] + b[t][u + 1] - lnp)
        return g


def batch_nll_grad(z, txt, enc_len, txt_len, blank=0, weight=None, use_autograd=True):
    """z [B, T, U+1, V] (any float dtype; float64 for the reference), padded txt [B, L] -> (nll [B], d (sum_b
    weight_b nll_b) / dz with exact zeros outside each utterance's lattice).  use_autograd: the alpha recursion under
    autograd (the differentiable path); otherwise the closed form."""
    B = z.shape[0]
    nll = []
    grad = torch.zeros_like(z)
    for b in range(B):
        Tb, Ub = int(enc_len[b]), int(txt_len[b])
        y = txt[b, :Ub].long()
        zb = z[b, :Tb, :Ub + 1].detach().clone()
        w = 1.0 if weight is None else float(weight[b])
        if use_autograd:
            zb.requires_grad_(True)
            n = -alpha_lnp(log_probs(zb), y, blank)
            n.backward()
            grad[b, :Tb, :Ub + 1] = zb.grad * w
        else:
            n = -alpha_lnp(log_probs(zb), y, blank)
            grad[b, :Tb, :Ub + 1] = closed_form(zb, y, blank) * w
        nll.append(n.detach())
    return torch.stack(nll), grad


# ---- the head ------------------------------------------------------------------------------------------------------------
class HeadRef(torch.nn.Module):
    """float64 mirror of TransducerHead on plain torch modules; `load(head)` copies the head's weights"""

    def __init__(self, vocab_size, enc_dim, module, dim, layer, emb_dim, joint_dim):
        super().__init__()
        self.module, self.layer, self.dim = module, layer, dim
        self.emb = torch.nn.Embedding(vocab_size, emb_dim)
        self.rnn = getattr(torch.nn, module)(emb_dim, dim, num_layers=layer, batch_first=True)
        self.lin_enc = torch.nn.Linear(enc_dim, joint_dim)
        self.lin_pred = torch.nn.Linear(dim, joint_dim)
        self.lin_out = torch.nn.Linear(joint_dim, vocab_size)
        self.double()

    def load(self, head):
        sd = {k: v.detach().cpu().double() for k, v in head.state_dict().items()}
        own = {"emb.weight": sd["emb.weight"]}
        for name in ("lin_enc", "lin_pred", "lin_out"):
            own[name + ".weight"] = sd[name + ".weight"]
            own[name + ".bias"] = sd[name + ".bias"]
        for l in range(self.layer):
            for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                own["rnn.%s_l%d" % (k, l)] = sd["pred.%s_l%d" % (k, l)]
        assert len(own) == len(sd), "the head has parameters the mirror does not know"
        self.load_state_dict(own, strict=True)
        return self

    def param_map(self):
        """name in the head's state_dict -> this mirror's parameter"""
        m = {"emb.weight": self.emb.weight}
        for name in ("lin_enc", "lin_pred", "lin_out"):
            m[name + ".weight"] = getattr(self, name).weight
            m[name + ".bias"] = getattr(self, name).bias
        for l in range(self.layer):
            for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                m["pred.%s_l%d" % (k, l)] = getattr(self.rnn, "%s_l%d" % (k, l))
        return m

    def logits(self, enc, txt):
        """enc [B, T, D] float64, txt [B, U] -> [B, T, U+1, V]; the prediction network reads <sos> = 0, then txt"""
        B = enc.shape[0]
        inp = torch.cat([txt.new_zeros((B, 1)), txt], dim=1)
        pred, _ = self.rnn(self.emb(inp))
        h = torch.tanh(self.lin_enc(enc).unsqueeze(2) + self.lin_pred(pred).unsqueeze(1))
        return self.lin_out(h)

    @classmethod
    def of(cls, head, enc_dim):
        return cls(head.vocab_size, enc_dim, head.rnn_type, head.dim, head.layer, head.emb_dim,
                   head.joint_dim).load(head)

    @torch.no_grad()
    def greedy(self, enc, max_symbols, max_len, blank=0):
        """one utterance enc [T, D] -> (tokens, trace): trace holds per decision (frame, argmax, margin between the best
        and the second-best logit, whether it emitted, whether the max_symbols cap alone kept it from emitting)"""
        T = enc.shape[0]
        fe = self.lin_enc(enc)
        tokens, trace = [], []
        last, state = 0, None
        out, new_state = self.rnn(self.emb(torch.tensor([[last]])), state)
        t = n_sym = 0
        while t < T:
            z = self.lin_out(torch.tanh(fe[t] + self.lin_pred(out[0, 0])))
            top = torch.topk(z, 2)
            k = int(top.indices[0])
            emit = not (k == blank or n_sym >= max_symbols or len(tokens) >= max_len)
            capped = k != blank and n_sym >= max_symbols and len(tokens) < max_len      # max_symbols alone stopped it
            trace.append((t, k, float(top.values[0] - top.values[1]), emit, capped))
            if emit:
                tokens.append(k)
                n_sym += 1
                state = new_state
                out, new_state = self.rnn(self.emb(torch.tensor([[k]])), state)
            else:
                t += 1
                n_sym = 0
        return tokens, trace


# ---- the cases of the greedy comparison -------------------------------------------------------------------------------------
GREEDY_V, GREEDY_ENC_DIM, GREEDY_LENS = 11, 16, (9, 5, 7)
GREEDY_MAX_SYMBOLS, GREEDY_MAX_LEN = 2, 6
MIN_MARGIN = 1e-3
# (prediction network, layers, seed, blank bias): seeds for which the float64 reference alone meets check_greedy_case
GREEDY_CASES = [("LSTM", 1, 0, 0.5), ("GRU", 2, 0, 0.5)]


def greedy_case(head_cls, module, layer, seed, blank_bias):
    """-> (head on the host, enc [3, 9, 16] f32, lens): a seeded head with widened output weights (decisive margins) and
    the blank's output bias set, and seeded encoder output with zero tails"""
    torch.manual_seed(seed)
    head = head_cls(GREEDY_V, GREEDY_ENC_DIM, dict(module=module, dim=12, layer=layer, emb_dim=20, dropout=0), 16)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        head.lin_out.weight.mul_(4.0)
        head.lin_enc.weight.mul_(3.0)
        head.lin_out.bias.zero_()
        head.lin_out.bias[0] = blank_bias
    enc = torch.randn((len(GREEDY_LENS), max(GREEDY_LENS), GREEDY_ENC_DIM), generator=g)
    for b, n in enumerate(GREEDY_LENS):
        enc[b, n:] = 0
    return head, enc, torch.tensor(GREEDY_LENS)


def check_greedy_case(ref, enc, lens):
    """the reference side of the greedy comparison, asserted before anything is compared: every decision has a margin of
    at least MIN_MARGIN, blanks and non-blanks occur, the max_symbols cap is hit, the rows finish at different iterations.
    -> the reference tokens per utterance"""
    out, n_iter, traces = [], [], []
    for b in range(enc.shape[0]):
        tokens, trace = ref.greedy(enc[b, :int(lens[b])].double(), GREEDY_MAX_SYMBOLS, GREEDY_MAX_LEN)
        out.append(tokens)
        n_iter.append(len(trace))
        traces += trace
    assert min(tr[2] for tr in traces) >= MIN_MARGIN, min(tr[2] for tr in traces)
    assert any(tr[1] == 0 for tr in traces), "no blank"
    assert any(tr[3] for tr in traces), "nothing emitted"
    assert any(tr[4] for tr in traces), "the max_symbols cap was never hit"
    assert len(set(n_iter)) == len(n_iter), n_iter
    return out
