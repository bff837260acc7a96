"""Float64 references, written from the definitions, and the case tables of the loss kernels: the CTC lattices and their
gradient (csrc/ctc.hip), the plain cross entropy, log-softmax and tanh (csrc/rowops.hip).

tests/test_loss_reference_cpu.py holds the references to torch's float64 CPU ops and every row to its input condition;
tests/test_loss_plan_cpu.py holds every CTC row to the launch plan it names (asrk_ctc_loss_plan_info);
tests/test_loss_variants_gpu.py runs every row on the device.  No GPU, no library call in this module.

CTC, over the blank-extended labels ext (blank on even states, target[(s-1)/2] on odd ones, S_b = 2 L_b + 1),
T_b = clamp(input_length, 0, T), L_b = min(target_length, Lmax):
    alpha_0[s] = lp_0[ext[s]] for s <= 1, -inf beyond
    alpha_t[s] = logsumexp(alpha_{t-1}[s], alpha_{t-1}[s-1], alpha_{t-1}[s-2] if s odd and ext[s] != ext[s-2]) + lp_t[ext[s]]
    beta the same from the other end; nll = -logsumexp(alpha_{T_b-1}[S-1], alpha_{T_b-1}[S-2])
    grad[t,b,c] = (exp(lp) - sum_{s: ext[s] = c} exp(alpha_t[s] + beta_t[s] + nll - lp)) * gscale[b] for t < T_b, else 0
(the gradient ATen's ctc_loss passes to a log-softmax: an empty sum is 0).  What the library documents beyond torch:
    T_b == 0: nll = 0 for an empty target, +inf otherwise, before any label is looked at;
    a label outside [0,V) among the first L_b: nll = NaN, gradient NaN for t < T_b and 0 beyond (include/asrk.h);
    nll = +inf (no path): with zero_infinity loss 0 and gradient 0; without it loss +inf, and the gradient of that
    utterance is NaN in its label columns (the blank's among them) and exp(lp) * gscale elsewhere (ops.CTCLossFn).
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
FLOOR = 4 * 2.0 ** -24


def bound(e32, factor, floor=FLOOR):
    """what a float32 kernel may be off by: `factor` times what the float32 CPU run of the same operation is off by on
    the same inputs, and never less than a few float32 roundings of the largest element"""
    return max(factor * e32, floor)


# hard limits: what the suite already holds each op to (tests/test_kernels_gpu.py, tests/test_loss_options_gpu.py)
HARD = dict(ctc_loss=1e-4, ctc_lattice=1e-4, ctc_grad=1e-3, ce_loss=1e-4, ce_grad=1e-3, lsm_y=2e-5, lsm_dx=1e-4)
TANH_ULP = 4


def finite_rel_err(a, b):
    """helpers.rel_err over the elements where the reference is finite (the others are compared exactly elsewhere)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = np.isfinite(b)
    if not m.any():
        return 0.0
    return float(np.max(np.abs(a[m] - b[m])) / max(float(np.max(np.abs(b[m]))), 1e-12))


def same_nonfinite(a, b):
    """NaN, +inf and -inf sit at the same places"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a == np.inf, b == np.inf)
                and np.array_equal(a == -np.inf, b == -np.inf))


# ====================================================================================================== CTC
def ctc_reference(lp, targets, in_len, tg_len, blank, gscale=None, zero_infinity=False, dtype=np.float64):
    """lp [T,B,V], targets [B,Lmax], lengths [B] -> dict(nll [B], loss [B], grad [T,B,V], alpha, beta (lists of
    [T_b,S_b] or None)).  loss is nll with the zero_infinity rule applied; grad is scaled by gscale [B] (default 1)."""
    lp = np.asarray(lp, dtype)
    T, B, V = lp.shape
    targets = np.asarray(targets, np.int64).reshape(B, -1)
    Lmax = targets.shape[1]
    gscale = np.ones(B, dtype) if gscale is None else np.asarray(gscale, dtype)
    nll = np.zeros(B, dtype)
    grad = np.zeros((T, B, V), dtype)
    alphas, betas = [], []
    ninf = dtype(-np.inf)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for b in range(B):
            Tb = max(min(int(in_len[b]), T), 0)
            L = min(int(tg_len[b]), Lmax)
            S = 2 * L + 1
            alphas.append(None)
            betas.append(None)
            if Tb == 0:
                nll[b] = 0.0 if L == 0 else np.inf
                continue
            lab = targets[b, :L]
            if ((lab < 0) | (lab >= V)).any():
                nll[b] = np.nan
                grad[:Tb, b, :] = np.nan
                continue
            ext = np.full(S, blank, np.int64)
            ext[1::2] = lab
            skip = np.zeros(S, bool)                    # alpha: may come from s-2
            skip[3::2] = ext[3::2] != ext[1:-2:2]
            skipb = np.zeros(S, bool)                   # beta: may go to s+2
            skipb[1:-2:2] = skip[3::2]
            g = lp[:Tb, b, :][:, ext]                   # [Tb,S]
            al = np.full((Tb, S), ninf, dtype)
            be = np.full((Tb, S), ninf, dtype)
            al[0, :2] = g[0, :2]
            be[Tb - 1, -2:] = g[Tb - 1, -2:]

            def shifted(p, k):                          # p[s - k], -inf where there is no such state
                out = np.full(S, ninf, dtype)
                if k > 0:
                    out[k:] = p[:max(S - k, 0)]
                else:
                    out[:max(S + k, 0)] = p[-k:]
                return out
            for t in range(1, Tb):
                p = al[t - 1]
                al[t] = np.logaddexp(np.logaddexp(p, shifted(p, 1)), np.where(skip, shifted(p, 2), ninf)) + g[t]
            for t in range(Tb - 2, -1, -1):
                p = be[t + 1]
                be[t] = np.logaddexp(np.logaddexp(p, shifted(p, -1)), np.where(skipb, shifted(p, -2), ninf)) + g[t]
            alphas[-1], betas[-1] = al, be
            end = al[Tb - 1, S - 1] if S < 2 else np.logaddexp(al[Tb - 1, S - 1], al[Tb - 1, S - 2])
            nll[b] = -end
            if nll[b] == np.inf and zero_infinity:
                continue
            x = lp[:Tb, b, :]
            gr = np.exp(x)
            lcab = np.full((Tb, V), ninf, dtype)
            ab = al + be
            for c in np.unique(ext):                    # log of the sum over the states that carry label c
                cols = ab[:, ext == c]
                m = cols.max(axis=1)
                ms = np.where(np.isfinite(m), m, 0.0)
                lcab[:, c] = ms + np.log(np.exp(cols - ms[:, None]).sum(axis=1))
            used = np.zeros(V, bool)
            used[ext] = True
            gr[:, used] -= np.exp(lcab[:, used] + nll[b] - x[:, used])     # -inf + inf = NaN where there is no path
            grad[:Tb, b, :] = gr * gscale[b]
    loss = nll.copy()
    if zero_infinity:
        loss[nll == np.inf] = 0.0
    return dict(nll=nll, loss=loss, grad=grad, alpha=alphas, beta=betas)


def ctc_reduce(loss, tg_len, Lmax, reduction, w, dtype=np.float64):
    """-> (what CTCLoss returns, gscale [B] of `(returned * w).sum().backward()`): w is [B] for 'none', a scalar else.
    'mean' divides every utterance by its clamped target length (at least 1) and by B, as torch does."""
    loss = np.asarray(loss, dtype)
    B = loss.shape[0]
    if reduction == 'none':
        return loss, np.asarray(w, dtype) * np.ones(B, dtype)
    if reduction == 'sum':
        return loss.sum(), np.full(B, w, dtype)
    n = np.clip(np.minimum(np.asarray(tg_len), Lmax), 1, None).astype(dtype)
    return (loss / n).mean(), np.asarray(w, dtype) / (n * B)


# ------------------------------------------------------------------------------------------------ the CTC table
# route = (states-per-lane template, FAST) of ctc_lattice_kernel; plan = fields of asrk_ctc_loss_plan_info the row is
# there for.  layout: 'tbv' contiguous [T,B,V]; 'btv' the transposed view of a [B,T,V] tensor; 'pad' a [:, :, :V] view of
# a [T,B,V+1] allocation (V % 4 == 0: 16-byte and scalar rows in one launch); 'off1' contiguous, one float into its
# allocation.  bias: how far the logits lean towards an alignment of the target (keeps nll small enough for the row's
# float32 CPU run to stay four times inside the hard limits); scale multiplies the random logits.
PLAN_FIELDS = ('tmpl', 'fast', 'spl', 'gather_y', 't_per_block', 'tchunks', 'dense_grid', 'smax')
PLAN_LEN = 8

CtcCase = collections.namedtuple('CtcCase', 'name T B V Lmax blank in_len tg_len route plan layout reduction zero_inf '
                                            'targets alphabet bias scale seed')


def _ctc(name, T, B, V, Lmax, in_len, tg_len, route, plan=None, blank=0, layout='tbv', reduction='none', zero_inf=False,
         targets=None, alphabet=None, bias=0.0, scale=1.0, seed=0):
    assert len(in_len) == B and len(tg_len) == B
    return CtcCase(name, T, B, V, Lmax, blank, tuple(in_len), tuple(tg_len), route, dict(plan or {}), layout, reduction,
                   zero_inf, targets, alphabet, bias, scale, seed)


_INF_IL, _INF_TL = [0, 0, 12, 3, 12, 4], [0, 2, 3, 3, 0, 4]
_INF_TG = [[1, 2, 3, 4], [1, 2, 3, 4], [5, 6, 1, 0], [2, 2, 3, 0], [1, 1, 1, 1], [4, 4, 4, 4]]
INFEASIBLE = (1, 3, 5)           # no frame; a repeat one frame short; three repeats in four frames

CTC_CASES = [
    # the eight-row prefetch ring: T_b on both sides of 1, CTC_PF = 8 and 2 x CTC_PF
    _ctc('ring_edges', 17, 8, 7, 3, [1, 2, 7, 8, 9, 10, 16, 17], [1, 1, 3, 3, 2, 3, 0, 3], (4, True), dict(spl=1)),
    # every instantiation at the boundary where spl and the template change; the short utterances leave lanes empty
    _ctc('l127', 160, 3, 12, 127, [160, 150, 90], [127, 60, 2], (4, True), dict(spl=4, smax=255), bias=3.0),
    _ctc('l128', 160, 3, 12, 128, [160, 150, 90], [128, 60, 2], (16, False), dict(spl=5, smax=257), bias=3.0),
    _ctc('l511', 560, 3, 12, 511, [560, 300, 560], [511, 255, 2], (16, False), dict(spl=16, smax=1023), bias=5.0),
    _ctc('l512', 560, 3, 12, 512, [560, 300, 560], [512, 256, 2], (32, False), dict(spl=17, smax=1025), bias=5.0),
    _ctc('t513_l3', 513, 2, 8, 3, [513, 400], [3, 2], (4, False), dict(spl=1, gather_y=65), bias=5.0),
    _ctc('t512_l3', 512, 2, 8, 3, [512, 400], [3, 2], (4, True), dict(spl=1, gather_y=64), bias=5.0),
    # the blank somewhere else
    _ctc('blank_last', 20, 3, 6, 4, [20, 13, 9], [4, 3, 0], (4, True), blank=5),
    _ctc('blank_mid', 20, 3, 7, 4, [20, 13, 9], [4, 3, 1], (4, True), blank=2),
    # targets that contain the blank's own index.  torch's CPU backward ASSIGNS the last frame's two end states to their
    # columns instead of adding them, so where the LAST label is the blank it loses one of the two terms of the blank
    # column at t = T_b - 1: the first two rows end on another label and agree with torch everywhere, the third ends on
    # the blank and is held to the definition there (TORCH_LAST_FRAME)
    _ctc('label_is_blank', 14, 4, 6, 3, [14, 10, 7, 14], [3, 3, 2, 3], (4, True),
         targets=[[1, 0, 2], [0, 0, 1], [0, 3, 0], [0, 4, 1]]),
    _ctc('label_is_blank_mid', 14, 3, 6, 3, [14, 10, 9], [3, 3, 3], (4, True), blank=3,
         targets=[[1, 3, 2], [3, 3, 1], [3, 4, 1]]),
    _ctc('label_is_blank_last', 14, 3, 6, 3, [14, 10, 7], [3, 3, 2], (4, True),
         targets=[[1, 2, 0], [0, 0, 0], [3, 0, 0]]),
    # a two-symbol alphabet: long chains of states with the same label in the gradient kernel
    _ctc('repeats', 40, 3, 3, 12, [40, 31, 26], [12, 9, 12], (4, True), alphabet=(1, 2), seed=3),
    # no labels at all
    _ctc('no_labels', 10, 3, 5, 0, [10, 5, 0], [0, 0, 0], (4, True), dict(spl=1, smax=1)),
    # gradient chunks
    _ctc('chunk_b1_t9', 9, 1, 5, 2, [5], [2], (4, True), dict(t_per_block=4, tchunks=3)),
    _ctc('b600_t6', 6, 600, 5, 2, [1 + (b * 7) % 6 for b in range(600)], [(b % 3) if (b * 7) % 6 else (b % 2) for b in range(600)],
         (4, True), dict(t_per_block=8, tchunks=1, dense_grid=900)),
    _ctc('b601_t5', 5, 601, 5, 1, [1 + (b * 3) % 5 for b in range(601)], [b % 2 for b in range(601)],
         (4, True), dict(t_per_block=8, tchunks=1, dense_grid=752)),      # 3005 rows: the last workgroup has one
    # layouts
    _ctc('lay_tbv', 11, 3, 8, 3, [11, 8, 5], [3, 2, 1], (4, True), layout='tbv'),
    _ctc('lay_btv', 11, 3, 8, 3, [11, 8, 5], [3, 2, 1], (4, True), layout='btv'),
    _ctc('lay_pad', 11, 3, 8, 3, [11, 8, 5], [3, 2, 1], (4, True), layout='pad'),
    _ctc('lay_off1', 11, 3, 8, 3, [11, 8, 5], [3, 2, 1], (4, True), layout='off1'),
    _ctc('lay_v7', 11, 3, 7, 3, [11, 8, 5], [3, 2, 1], (4, True), layout='tbv'),
    _ctc('lay_v7_btv', 11, 3, 7, 3, [11, 8, 5], [3, 2, 1], (4, True), layout='btv'),
    # peaky posteriors: log-probs down to about -60
    _ctc('peaky', 30, 3, 8, 4, [30, 22, 12], [4, 4, 2], (4, True), scale=12.0, bias=20.0),
]
for _zi in (False, True):
    for _red in ('none', 'mean', 'sum'):
        # input_length 0 with an empty and a non-empty target, infeasible utterances beside feasible ones
        CTC_CASES.append(_ctc('inf_%s_%s' % (_red, 'zero' if _zi else 'keep'), 12, 6, 7, 4, _INF_IL, _INF_TL, (4, True),
                              reduction=_red, zero_inf=_zi, targets=_INF_TG))
CTC_BY_NAME = {c.name: c for c in CTC_CASES}
TORCH_LAST_FRAME = ('label_is_blank_last',)
assert len(CTC_BY_NAME) == len(CTC_CASES)

# rows torch rejects: asserted against the documented semantics
# labels -3 and V + 100: as column indices they would land before the gradient tensor (utterance 0), in other utterances'
# rows and up to 88 floats past its end (utterance 2 at the last frame); the 999 of utterance 3 lies beyond its length
BAD_LABELS = _ctc('bad_labels', 9, 5, 6, 3, [9, 7, 9, 5, 6], [3, 3, 3, 2, 3], (4, True),
                  targets=[[1, -3, 2], [1, 2, 3], [4, 106, 1], [2, 5, 999], [1, 1, -3]])
BAD_UTTS = (0, 2, 4)
GOOD_UTTS = (1, 3)
# lengths beyond the tensor: clamp to [11, 11, 11] / [3, 3, 2]
LEN_BEYOND = [_ctc('len_beyond_' + red, 11, 3, 8, 3, [14, 11, 300], [3, 7, 2], (4, True), reduction=red)
              for red in ('none', 'mean', 'sum')]
ALL_CTC = CTC_CASES + [BAD_LABELS] + LEN_BEYOND


def ctc_weights(c):
    """the factor of `(loss * w).sum().backward()`: one per utterance for 'none', a scalar else"""
    if c.reduction == 'none':
        return np.asarray([1.0 + 0.25 * (b % 5) for b in range(c.B)], np.float32)
    return np.float32(1.3)


def ctc_targets(c):
    g = np.random.RandomState(1000 + c.seed)
    if c.targets is not None:
        return np.asarray(c.targets, np.int64).reshape(c.B, c.Lmax)
    labels = [v for v in (c.alphabet or range(c.V)) if v != c.blank]
    tg = np.zeros((c.B, c.Lmax), np.int64)
    for b in range(c.B):
        prev = -1
        for i in range(c.Lmax):
            # long targets never repeat a label (every repeat costs a frame, and T is only just above L there)
            pool = [v for v in labels if v != prev] if c.Lmax > 64 else labels
            prev = pool[g.randint(len(pool))]
            tg[b, i] = prev
    return tg


@functools.lru_cache(maxsize=None)
def _ctc_inputs(name):
    c = {x.name: x for x in ALL_CTC}[name]
    g = torch.Generator().manual_seed(77 + c.seed + 13 * c.T + c.Lmax)
    logits = torch.randn((c.T, c.B, c.V), generator=g, dtype=F64) * c.scale
    tg = ctc_targets(c)
    if c.bias:
        for b in range(c.B):
            Tb, L = max(min(c.in_len[b], c.T), 1), min(c.tg_len[b], c.Lmax)
            lab = np.clip(tg[b, :L], 0, c.V - 1)
            for t in range(Tb):
                # an alignment: label i holds frames [i Tb / L, (i+1) Tb / L); a repeated label starts with a blank
                col = c.blank
                if L > 0:
                    i = min(t * L // Tb, L - 1)
                    first = t == 0 or (t - 1) * L // Tb != i
                    if not (first and i > 0 and lab[i] == lab[i - 1]):
                        col = int(lab[i])
                logits[t, b, col] += c.bias
    lp = logits.log_softmax(-1).to(torch.float32)          # the float32 values every run starts from
    return lp, torch.from_numpy(tg), torch.tensor(c.in_len, dtype=torch.int64), torch.tensor(c.tg_len, dtype=torch.int64)


def ctc_inputs(c):
    """-> lp [T,B,V] float32 (contiguous, CPU), targets [B,Lmax], input_lengths, target_lengths; cached, never modify"""
    return _ctc_inputs(c.name)


def ctc_layout(c, lp, device):
    """lp [T,B,V] CPU -> the row's view of it on `device`"""
    T, B, V = lp.shape
    if c.layout == 'tbv':
        return lp.to(device).contiguous()
    if c.layout == 'btv':
        return lp.transpose(0, 1).contiguous().to(device).transpose(0, 1)
    if c.layout == 'pad':
        big = torch.full((T, B, V + 1), 7.0, dtype=torch.float32, device=device)
        big[:, :, :V] = lp.to(device)
        return big[:, :, :V]
    assert c.layout == 'off1'
    big = torch.full((T * B * V + 4,), 7.0, dtype=torch.float32, device=device)
    big[1:1 + T * B * V] = lp.to(device).reshape(-1)
    return big[1:1 + T * B * V].view(T, B, V)


@functools.lru_cache(maxsize=None)
def _ctc_expected(name):
    c = {x.name: x for x in ALL_CTC}[name]
    lp, tg, il, tl = ctc_inputs(c)
    w = ctc_weights(c)
    plain = ctc_reference(lp.numpy(), tg.numpy(), il.numpy(), tl.numpy(), c.blank, zero_infinity=c.zero_inf)
    out, gscale = ctc_reduce(plain['loss'], tl.numpy(), c.Lmax, c.reduction, w)
    full = ctc_reference(lp.numpy(), tg.numpy(), il.numpy(), tl.numpy(), c.blank, gscale=gscale, zero_infinity=c.zero_inf)
    return dict(nll=full['nll'], out=np.asarray(out), grad=full['grad'], gscale=gscale, alpha=full['alpha'],
                beta=full['beta'])


def ctc_expected(c):
    """float64: nll [B], out (what CTCLoss returns), grad [T,B,V] of (out * w).sum(), gscale [B]; cached"""
    return _ctc_expected(c.name)


def ctc_torch_args(c):
    """the row as torch's CPU ctc_loss accepts it: lengths clamped as the kernels clamp them"""
    lp, tg, il, tl = ctc_inputs(c)
    return lp, tg, il.clamp(0, c.T), tl.clamp(max=c.Lmax)


def ctc_torch(c, dtype, utts=None):
    """F.ctc_loss on the CPU in `dtype` -> (out, grad of (out * w).sum()) as numpy; utts: only these utterances"""
    lp, tg, il, tl = ctc_torch_args(c)
    w = torch.as_tensor(ctc_weights(c)).to(dtype)
    if utts is not None:
        assert c.reduction == 'none'
        utts = list(utts)
        lp, tg, il, tl, w = lp[:, utts], tg[utts], il[utts], tl[utts], w[utts]
    x = lp.clone().to(dtype).requires_grad_(True)
    out = F.ctc_loss(x, tg, il, tl, blank=c.blank, reduction=c.reduction, zero_infinity=c.zero_inf)
    (out * w).sum().backward()
    return out.detach().numpy(), x.grad.numpy()


def ctc_grad_err(got, ref):
    """helpers.rel_err of a [T,B,V] gradient; where the reference has utterances that are not finite, the largest
    rel_err over the utterances that are (a norm over the whole tensor is NaN there)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if np.isfinite(ref).all():
        return finite_rel_err(got, ref)
    ok = [b for b in range(ref.shape[1]) if np.isfinite(ref[:, b]).all()]
    return max([float(np.max(np.abs(got[:, b] - ref[:, b])) / max(float(np.max(np.abs(ref[:, b]))), 1e-12)) for b in ok]
               + [0.0])


@functools.lru_cache(maxsize=None)
def _ctc_e32(name, utts=None):
    c = {x.name: x for x in ALL_CTC}[name]
    o64, g64 = ctc_torch(c, F64, utts)
    o32, g32 = ctc_torch(c, torch.float32, utts)
    return dict(ctc_loss=finite_rel_err(o32, o64), ctc_grad=ctc_grad_err(g32, g64))


def ctc_e32(c, utts=None):
    """what the float32 CPU run of torch's op is off by against its float64 run, per tensor kind (utts: of these
    utterances alone, for a row with utterances torch rejects)"""
    return _ctc_e32(c.name, None if utts is None else tuple(utts))


LATTICE_ROWS = ('ring_edges', 'label_is_blank', 't513_l3', 'l128', 'l512')       # one per instantiation and more


def lattice_err(got, ref):
    """got, ref: per utterance [T_b,S_b] or None -> the largest finite_rel_err over the utterances; the -inf of the
    states no path reaches must sit at the same places"""
    worst = 0.0
    for a, r in zip(got, ref):
        if r is None:
            continue
        assert same_nonfinite(a, r)
        worst = max(worst, finite_rel_err(a, r))
    return worst


@functools.lru_cache(maxsize=None)
def _ctc_lattice_e32(name):
    c = CTC_BY_NAME[name]
    lp, tg, il, tl = ctc_inputs(c)
    r32 = ctc_reference(lp.numpy(), tg.numpy(), il.numpy(), tl.numpy(), c.blank, dtype=np.float32)
    r64 = ctc_expected(c)
    return max(lattice_err(r32['alpha'], r64['alpha']), lattice_err(r32['beta'], r64['beta']))


def ctc_lattice_e32(c):
    """alpha and beta are not torch's to show: the float32 run of this module's own recursion against its float64 run"""
    return _ctc_lattice_e32(c.name)


# ====================================================================================================== cross entropy
def ce_reference(x, t, ignore_index, w=1.0, dtype=F64):
    """x [R,V], t [R] -> (mean loss over the counted rows, d (loss * w) / dx).  A row counts if its target is not
    ignore_index and lies in [0,V); no counted row gives 0 / 0 = NaN and a zero gradient."""
    x = x.to(dtype)
    R, V = x.shape
    live = (t != ignore_index) & (t >= 0) & (t < V)
    m = x.max(dim=1, keepdim=True).values
    lse = m.squeeze(1) + (x - m).exp().sum(1).log()
    tc = t.clamp(0, V - 1)
    row = lse - x[torch.arange(R), tc]
    n = int(live.sum())
    loss = row[live].sum() / n if n else torch.tensor(float('nan'), dtype=dtype)
    dx = torch.zeros_like(x)
    if n:
        p = (x - lse[:, None]).exp()
        p[torch.arange(R), tc] -= 1.0
        dx[live] = p[live] * (w / n)
    return loss, dx


CeCase = collections.namedtuple('CeCase', 'name R V ignore values oob all_ignored')
CE_SIZES_V = (1, 3, 63, 64, 65, 4100)
CE_SIZES_R = (1, 4, 5, 257)


def _ce_cases():
    out, k = [], 0
    for V in CE_SIZES_V:
        for R in CE_SIZES_R:
            ign = (0, -100, 'mid')[k % 3]
            k += 1
            if V == 1:
                ign = -100                              # the only class would be the ignored one
            out.append(CeCase('v%d_r%d_ign%s' % (V, R, ign), R, V, V // 2 if ign == 'mid' else ign, 'randn', R >= 4, False))
    for ign in (0, -100, 32):
        out.append(CeCase('oob_ign%d' % ign, 9, 65, ign, 'randn', True, False))
        out.append(CeCase('all_ignored_ign%d' % ign, 6, 65, ign, 'randn', True, True))
    for v in ('offset', 'constant', 'ninf_other', 'ninf_target'):
        out.append(CeCase(v, 5, 65, 0, v, False, False))
    for V, R, ign in ((64, 5, -100), (65, 4, 0), (3, 5, 1), (4100, 4, 0)):
        out.append(CeCase('ld_v%d' % V, R, V, ign, 'randn', True, False))
    return out


CE_CASES = _ce_cases()
CE_BY_NAME = {c.name: c for c in CE_CASES}
assert len(CE_BY_NAME) == len(CE_CASES)
# through the C ABI with a leading dimension above V: (row, ld - V)
CE_LD_CASES = [(c.name, pad) for c in CE_CASES if c.name.startswith('ld_') for pad in (3, 4)]
CE_DET_ROWS = (1, 255, 256, 257, 600)
CE_DET_V = 37
CE_W = 1.7


@functools.lru_cache(maxsize=None)
def _ce_inputs(name):
    c = CE_BY_NAME[name] if name in CE_BY_NAME else None
    if c is None:                                       # the deterministic-mode rows: 'det_<rows>'
        c = CeCase(name, int(name.split('_')[1]), CE_DET_V, 0, 'randn', False, False)
    g = torch.Generator().manual_seed(500 + 7 * c.R + c.V)
    x = torch.randn((c.R, c.V), generator=g) * 2.0
    if c.V > 1:
        t = torch.randint(1 if c.ignore == 0 else 0, c.V, (c.R,), generator=g)
        if c.ignore != -100 and c.ignore != 0:
            t[t == c.ignore] = (c.ignore + 1) % c.V
    else:
        t = torch.zeros((c.R,), dtype=torch.int64)
    if c.R >= 3:
        t[torch.arange(c.R) % 3 == 1] = c.ignore        # about a third of the rows are ignored
    if c.oob:
        for i, v in zip(range(0, c.R, 4), (-1, c.V, c.V + 7)):
            t[i] = v                                    # torch raises on these; here they are ignored rows
    if c.all_ignored:
        t[torch.arange(c.R) % 2 == 0] = c.ignore
        t[torch.arange(c.R) % 4 == 1] = c.V + 7
        t[torch.arange(c.R) % 4 == 3] = -1
    if c.values == 'offset':
        x[0] += 80.0
        x[1] -= 80.0
        x[2] += 80.0 * torch.sign(torch.randn(c.V, generator=g))      # +-80 inside one row
    elif c.values == 'constant':
        x[0] = 3.25
        x[2] = -80.0
    elif c.values in ('ninf_other', 'ninf_target'):
        for r in (0, 2, 3):
            cols = torch.randperm(c.V, generator=g)[:20]
            cols = cols[cols != t[r]]
            x[r, cols] = -float('inf')
        if c.values == 'ninf_target':
            x[2, t[2]] = -float('inf')                  # the loss of the batch is +inf
    return c, x, t


def ce_inputs(c_or_name):
    """-> (case, logits [R,V] float32, targets [R]); cached, never modify"""
    return _ce_inputs(c_or_name if isinstance(c_or_name, str) else c_or_name.name)


@functools.lru_cache(maxsize=None)
def _ce_expected(name):
    c, x, t = _ce_inputs(name)
    loss, dx = ce_reference(x, t, c.ignore, CE_W)
    return loss.numpy(), dx.numpy()


def ce_expected(c_or_name):
    return _ce_expected(c_or_name if isinstance(c_or_name, str) else c_or_name.name)


def ce_torch(c, x, t, dtype):
    """F.cross_entropy on the CPU; targets outside [0,V) become ignore_index first, which is what they mean here"""
    ts = torch.where((t >= 0) & (t < c.V), t, torch.full_like(t, c.ignore))
    xr = x.clone().to(dtype).requires_grad_(True)
    loss = F.cross_entropy(xr, ts, ignore_index=c.ignore)
    (loss * CE_W).backward()
    return loss.detach().numpy(), xr.grad.numpy()


@functools.lru_cache(maxsize=None)
def _ce_e32(name):
    c, x, t = _ce_inputs(name)
    l64, g64 = ce_torch(c, x, t, F64)
    l32, g32 = ce_torch(c, x, t, torch.float32)
    return dict(ce_loss=finite_rel_err(l32, l64), ce_grad=finite_rel_err(g32, g64))


def ce_e32(c_or_name):
    return _ce_e32(c_or_name if isinstance(c_or_name, str) else c_or_name.name)


# ====================================================================================================== log-softmax
def log_softmax_reference(x, dy=None, dtype=F64):
    """rows of x -> y = x - logsumexp(x) and, given dy, dx = dy - exp(y) * sum(dy).  A row of -inf alone is NaN."""
    x = x.to(dtype)
    m = x.max(dim=-1, keepdim=True).values
    y = x - (m + (x - m).exp().sum(-1, keepdim=True).log())
    if dy is None:
        return y, None
    dy = dy.to(dtype)
    return y, dy - y.exp() * dy.sum(-1, keepdim=True)


LsmCase = collections.namedtuple('LsmCase', 'name rows cols values')
LSM_COLS = (1, 3, 4, 252, 256, 260, 5000)
LSM_ROWS = (1, 4, 5)
LSM_CASES = [LsmCase('c%d_r%d' % (cols, rows), rows, cols, 'randn') for cols in LSM_COLS for rows in LSM_ROWS]
LSM_CASES += [LsmCase('extremes', 5, 260, 'extremes'), LsmCase('extremes_odd', 5, 63, 'extremes')]
LSM_BY_NAME = {c.name: c for c in LSM_CASES}
# through the C ABI: (row, ld - cols, floats the base is off a 16-byte boundary, the kernel that must run)
LSM_ABI = [('c256_r5', 0, 0, 'vector'), ('c256_r5', 4, 0, 'vector'), ('c256_r5', 1, 0, 'scalar'), ('c256_r5', 0, 1, 'scalar'),
           ('c260_r4', 4, 0, 'vector'), ('c260_r4', 1, 0, 'scalar'), ('c4_r5', 4, 1, 'scalar'), ('c3_r5', 1, 0, 'scalar'),
           ('c252_r1', 4, 0, 'vector'), ('extremes', 4, 0, 'vector'), ('extremes', 1, 1, 'scalar')]


def lsm_kernel(cols, ld, off):
    """asrk_log_softmax_{fwd,bwd}_f32's choice for 16-byte aligned allocations entered `off` floats in"""
    return 'vector' if off % 4 == 0 and cols % 4 == 0 and ld % 4 == 0 else 'scalar'


@functools.lru_cache(maxsize=None)
def _lsm_inputs(name):
    c = LSM_BY_NAME[name]
    g = torch.Generator().manual_seed(900 + 3 * c.rows + c.cols)
    x = torch.randn((c.rows, c.cols), generator=g) * 3.0
    dy = torch.randn((c.rows, c.cols), generator=g)
    if c.values == 'extremes':
        x[0] = x[0] - x[0].max() + 90.0                 # exp(90) overflows float32: only the shifted form survives
        x[1] = x[1] - x[1].max() - 90.0                 # exp(-90) underflows
        x[2, ::3] = -float('inf')
        x[3] = -float('inf')                            # NaN, as torch gives
    return x, dy


def lsm_inputs(c):
    return _lsm_inputs(c.name)


@functools.lru_cache(maxsize=None)
def _lsm_expected(name):
    y, dx = log_softmax_reference(*_lsm_inputs(name))
    return y.numpy(), dx.numpy()


def lsm_expected(c):
    return _lsm_expected(c.name)


def lsm_torch(c, dtype):
    x, dy = lsm_inputs(c)
    xr = x.clone().to(dtype).requires_grad_(True)
    y = F.log_softmax(xr, dim=-1)
    y.backward(dy.to(dtype))
    return y.detach().numpy(), xr.grad.numpy()


@functools.lru_cache(maxsize=None)
def _lsm_e32(name):
    c = LSM_BY_NAME[name]
    y64, d64 = lsm_torch(c, F64)
    y32, d32 = lsm_torch(c, torch.float32)
    return dict(lsm_y=finite_rel_err(y32, y64), lsm_dx=finite_rel_err(d32, d64))


def lsm_e32(c):
    return _lsm_e32(c.name)


# ====================================================================================================== tanh
def tanh_reference(x, dy=None, dtype=F64):
    """-> y = (e^x - e^-x) / (e^x + e^-x) in the form that does not overflow, and dx = dy * (1 - y32^2) where y32 is y
    rounded to float32: the backward reads the float32 y the forward stored"""
    x = x.to(dtype)
    e = (-2.0 * x.abs()).exp()
    y = torch.sign(x) * (1.0 - e) / (1.0 + e)
    small = x.abs() < 1e-5
    y = torch.where(small, x - x ** 3 / 3.0, y)          # (1 - e) cancels below: the series is exact to 1e-20 there
    if dy is None:
        return y, None
    y32 = y.to(torch.float32).to(dtype)
    return y, dy.to(dtype) * (1.0 - y32 * y32)


TANH_SIZES = (1, 255, 256, 257, 1048576 + 259)
TANH_SPECIAL = (0.0, -0.0, 1e-45, -1e-45, 5e-39, -5e-39, 1.1754944e-38, 9.0, -9.0, 100.0, -100.0, float('inf'),
                -float('inf'), float('nan'), 1e-3, -1e-3, 0.5, -0.5, 8.3, 19.0)


@functools.lru_cache(maxsize=None)
def tanh_inputs(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn((n,), generator=g) * 3.0
    dy = torch.randn((n,), generator=g)
    return x, dy


def tanh_special():
    return torch.tensor(TANH_SPECIAL, dtype=torch.float32)


def ulp_distance(a32, ref64):
    """units in the last place between float32 values and a float64 reference rounded to float32 (NaN against NaN: 0;
    +0 against -0: 0)"""
    a = np.asarray(a32, np.float32)
    r = np.asarray(ref64, np.float64).astype(np.float32)
    both_nan = np.isnan(a) & np.isnan(r)

    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(r))
    d[both_nan] = 0
    d[np.isnan(a) != np.isnan(r)] = 2 ** 31
    return d
