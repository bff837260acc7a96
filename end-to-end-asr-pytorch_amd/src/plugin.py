"""Word-embedding plug-in — mirror of the reference's src/plugin.py:7-160 (`EmbeddingRegularizer`: same constructor
kwargs, attributes, state_dict keys and `forward(dec_state, dec_logit, label, return_loss) -> (loss, log_fused_prob)`).

Two functions: the decoder state is regressed onto pretrained word embeddings (cosine embedding loss), and - with
`fuse != 0` - the decoder's softmax is replaced by a mixture of the decoder distribution and an embedding-similarity
distribution, in training and in beam search.

MI355X: the mixture, the cosine loss (target rows gathered inside the kernel) and the row normalisation are the kernels
of csrc/emb_fuse.hip (emb_ops.py); emb_net's linears and the embedding logits are ops.linear GEMMs.  The torch modules
held here (`emb_table`, `emb_net`) are parameter containers only - they fix the state_dict layout and the from-seed
initialisation order (emb_table, emb_net, fusion parameters) and are never called.

Deviations from the reference: `distance='MSE'` raises at construction (the reference crashes on its
first forward unless emb_dim == 1), `bert=` raises NotImplementedError (the BERT predictor is not built).
"""
import torch
from torch import nn

from .. import ops
from .. import emb_ops
from .. import decoder_ops as dops
from .util import load_embedding


class EmbeddingRegularizer(nn.Module):
    ''' Perform word embedding regularization training for ASR '''

    def __init__(self, tokenizer, dec_dim, enable, src, distance, weight, fuse, temperature,
                 freeze=True, fuse_normalize=False, dropout=0.0, bert=None):
        super().__init__()
        self.enable = enable
        if not enable:
            return
        if bert is not None:
            raise NotImplementedError('emb.bert: the BERT embedding predictor (src/bert_embedding.py) is not built')
        self.use_bert = False
        pretrained_emb = torch.FloatTensor(load_embedding(tokenizer, src))
        vocab_size, emb_dim = pretrained_emb.shape
        self.dim = emb_dim
        self.emb_table = nn.Embedding.from_pretrained(pretrained_emb, freeze=freeze, padding_idx=0)
        hid = (emb_dim + dec_dim) // 2
        self.emb_net = nn.Sequential(nn.Linear(dec_dim, hid), nn.ReLU(), nn.Linear(hid, emb_dim))
        self.weight = weight
        self.distance = distance
        self.fuse_normalize = fuse_normalize
        if distance == 'MSE':
            raise NotImplementedError("emb.distance 'MSE' is not supported: the reference fails on its first forward "
                                      "with it unless the embedding width is 1; use 'CosEmb'")
        if distance != 'CosEmb':
            raise NotImplementedError

        self.apply_dropout = dropout > 0
        self.dropout_p = float(dropout)

        self.apply_fuse = fuse != 0
        if self.apply_fuse:
            # weight for mixing the embedding / decoder distributions
            if fuse == -1:
                self.fuse_type = "learnable"
                self.fuse_learnable = True
                self.fuse_lambda = nn.Parameter(data=torch.FloatTensor([0.5]))
            elif fuse == -2:
                self.fuse_type = "vocab-wise learnable"
                self.fuse_learnable = True
                self.fuse_lambda = nn.Parameter(torch.ones((vocab_size)) * 0.5)
            else:
                self.fuse_type = str(fuse)
                self.fuse_learnable = False
                self.register_buffer('fuse_lambda', torch.FloatTensor([fuse]))
            # temperature of the embedding distribution
            if temperature == -1:
                self.temperature = 'learnable'
                self.temp = nn.Parameter(data=torch.FloatTensor([1]))
            elif temperature == -2:
                self.temperature = 'elementwise'
                self.temp = nn.Parameter(torch.ones((vocab_size)))
            else:
                self.temperature = str(temperature)
                self.register_buffer('temp', torch.FloatTensor([temperature]))
            self.eps = 1e-8
        self._norm_table = None     # normalised table of the no-autograd path, valid for one search

    def create_msg(self):
        msg = ['Plugin.    | Word embedding regularization enabled (type:{}, weight:{})'.format(
            self.distance, self.weight)]
        if self.apply_fuse:
            msg.append('           | Embedding-fusion decoder enabled ( temp. = {}, lambda = {} )'.
                       format(self.temperature, self.fuse_type))
        return msg

    def get_weight(self):
        if self.fuse_learnable:
            return torch.sigmoid(self.fuse_lambda).mean().cpu().data
        return self.fuse_lambda

    def get_temp(self):
        return nn.functional.relu(self.temp).mean()

    def _embed(self, dec_state):
        ''' emb_net: decoder state -> embedding space '''
        l0, l2 = self.emb_net[0], self.emb_net[2]
        return ops.linear(emb_ops.relu(ops.linear(dec_state, l0.weight, l0.bias)), l2.weight, l2.bias)

    def fuse_prob(self, x_emb, dec_logit):
        ''' log of the mixture of the decoder distribution and the embedding-similarity distribution '''
        table = self.emb_table.weight
        if self.fuse_normalize:
            x_emb, table = emb_ops.l2_normalize(x_emb), emb_ops.l2_normalize(table)
        emb_logit = ops.linear(x_emb, table)
        return emb_ops.fuse(dec_logit, emb_logit, self.temp, self.fuse_lambda, self.fuse_learnable, self.eps)

    def forward(self, dec_state, dec_logit, label=None, return_loss=True):
        log_fused_prob, loss = None, None
        if self.apply_dropout:
            dec_state = ops.dropout(dec_state, self.dropout_p, self.training)
        x_emb = self._embed(dec_state)
        if return_loss:
            # regression of the decoder state onto the label's embedding, padding masked out
            loss = emb_ops.cos_emb_loss(x_emb, self.emb_table.weight, label)
        if self.apply_fuse:
            log_fused_prob = self.fuse_prob(x_emb, dec_logit)
        return loss, log_fused_prob

    def begin_search(self):
        ''' the beam decoders call this at the start of every search: the normalised table kept by infer() is dropped
            (the table may have been updated in place since - the fused optimiser does not bump tensor versions) '''
        self._norm_table = None

    @torch.no_grad()
    def infer(self, dec_state, dec_logit):
        ''' beam-search entry: decoder states [n,D] and logits [n,V] -> fused log-probabilities [n,V]; no autograd
            node, no loss, dropout off.  The embedding logits go through decoder_ops.linear_infer, which takes the
            cached split panel of the table only from 128 rows and for an embedding width that is a multiple of 32
            (not the shipped 300) and is ops.linear otherwise. '''
        assert self.apply_fuse, 'embedding fusion is off (emb.fuse == 0)'
        l0, l2 = self.emb_net[0], self.emb_net[2]
        h = emb_ops.relu_(ops.linear(dec_state, l0.weight, l0.bias))
        x_emb = ops.linear(h, l2.weight, l2.bias)
        table = self.emb_table.weight
        if self.fuse_normalize:
            x_emb = emb_ops.l2_normalize_infer(x_emb)
            if self._norm_table is None:        # once per search (begin_search)
                self._norm_table = emb_ops.l2_normalize_infer(table)
            table = self._norm_table
        emb_logit = dops.linear_infer(x_emb, table) if x_emb.dim() == 2 else ops.linear(x_emb, table)
        return emb_ops.fuse(dec_logit, emb_logit, self.temp, self.fuse_lambda, self.fuse_learnable, self.eps)
