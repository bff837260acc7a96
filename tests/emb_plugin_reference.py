"""Plain-torch float64 restatement of the word-embedding plug-in's arithmetic: the yardstick of
tests/test_emb_plugin_gpu.py (the GPU machine has no reference checkout) and itself checked against the recorded
reference in tests/test_emb_plugin_cpu.py.  Written from the formulas, not from the kernels:

    a_v = max(temp_v, 0) * e_v,  pe = softmax(a),  pd = softmax(d),  s_v = sigmoid(lam_v) or lam_v
    y_v = log((1 - s_v) pd_v + s_v pe_v + eps)
    cosine row loss = 1 - x.y / sqrt((|x|^2 + 1e-12)(|y|^2 + 1e-12)), y = table[label], 0 where label == 0
    loss = mean_b(sum_t row loss / #{t: label != 0})
    nll = mean over t_n != ignore_index of -y[n, t_n]
    normalize(x) = x / max(|x|, 1e-12)

Gradients come from autograd on these float64 expressions."""
import torch

F64 = torch.float64


def _softmax(x):
    z = x - x.max(dim=-1, keepdim=True)[0]
    ez = z.exp()
    return ez / ez.sum(dim=-1, keepdim=True)


def fuse(dec_logit, emb_logit, temp, lam, lam_is_logit, eps=1e-8):
    a = temp.clamp(min=0) * emb_logit
    pe, pd = _softmax(a), _softmax(dec_logit)
    s = torch.sigmoid(lam) if lam_is_logit else lam
    return ((1 - s) * pd + s * pe + eps).log()


def cos_emb_loss(x, table, label):
    b, t = label.shape
    x = x.reshape(b * t, -1)
    y = table[label.reshape(-1)]
    cos = (x * y).sum(-1) / (((x * x).sum(-1) + 1e-12) * ((y * y).sum(-1) + 1e-12)).sqrt()
    row = torch.where(label.reshape(-1) != 0, 1 - cos, torch.zeros_like(cos)).reshape(b, t)
    return (row.sum(-1) / (label != 0).sum(-1).to(x.dtype)).mean()


def nll(logp, target, ignore_index=0):
    keep = target != ignore_index
    picked = logp[torch.arange(logp.shape[0]), target.clamp(min=0)]
    return -(picked * keep).sum() / keep.sum()


def normalize(x, eps=1e-12):
    return x / x.norm(dim=-1, keepdim=True).clamp(min=eps)


def plugin_forward(p, dec_state, dec_logit, label, fuse_on, learnable, fuse_normalize=False, eps=1e-8):
    """(loss, log_fused_prob | None) of the module with state_dict-like parameters `p` (float64 tensors)"""
    h = (dec_state @ p['emb_net.0.weight'].t() + p['emb_net.0.bias']).clamp(min=0)
    x_emb = h @ p['emb_net.2.weight'].t() + p['emb_net.2.bias']
    table = p['emb_table.weight']
    loss = cos_emb_loss(x_emb, table, label)
    fused = None
    if fuse_on:
        xe, tb = (normalize(x_emb), normalize(table)) if fuse_normalize else (x_emb, table)
        fused = fuse(dec_logit, xe @ tb.t(), p['temp'], p['fuse_lambda'], learnable, eps)
    return loss, fused
