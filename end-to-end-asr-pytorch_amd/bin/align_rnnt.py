"""Token times from the transducer head, for `main.py --test` with a `decode: {transducer: ...}` block.

`align: true`: every utterance of the dev and test sets is aligned to its REFERENCE transcript (ASR.transducer_align:
the best path through the transducer lattice, found and traced back on the device - csrc/rnnt_align.hip).  There is no
search and no LM.  Utterances go through in groups of `ASRK_DECODE_BATCH` (default 16), through the packed encoder where
the model has one (every utterance encoded as if alone, so grouping and padding never change an alignment; else one
utterance at a time), and fan out over ranks like the decoding modes (bin/test_asr.py: _my_share / gather_in_order).
Rank 0 writes, per set,

    <outdir>/<name>_{dev,test}_rnnt_align.tsv        idx, pos, token, frame, time_s, logp, post
                                                     one row per transcript token: the ENCODER frame at which it was
                                                     emitted, that frame's start in seconds, the token's log-probability
                                                     at the emitting cell and the posterior of that emission (the
                                                     per-token confidence)
    <outdir>/<name>_{dev,test}_rnnt_align_score.tsv  idx, score: log-probability of the best path (-inf: the transcript
                                                     does not fit; it then has no token rows)

`timestamps: true`: after the greedy or beam search the best hypothesis of every utterance is aligned by the same path
(ASR.transducer_align on the hypothesis, on the batch the search ran on) and <outdir>/<name>_{dev,test}_rnnt_times.tsv
receives the same columns beside the usual output, which does not change.  These are the Viterbi times of the
hypothesis, not the search's own emission steps: the search sums over alignments (beam) or commits frame by frame
(greedy), the times are those of the single best alignment of what it found.  An empty hypothesis writes no row.

seconds = frame x encoder subsampling x feature frame shift (align_asr.frame_seconds).
"""
import os

import torch

from . import test_asr
from .align_asr import SCORE_HEADER, frame_seconds, token_text
from ..parallel import gather_in_order

TIMES_HEADER = 'idx\tpos\ttoken\tframe\ttime_s\tlogp\tpost\n'


def token_rows(txt, n, frames, logp, post):
    ''' host lists of one utterance -> [(token id, frame, logp, post), ...], nothing when it has no path '''
    return [(txt[u], frames[u], logp[u], post[u]) for u in range(n) if frames[u] >= 0]


def align_tokens(model, feat, feat_len, txt, txt_len, packed=False):
    ''' one padded batch -> (score list, [token_rows per utterance]) '''
    frames, _, logp, post, score, _ = model.transducer_align(feat, feat_len, txt, txt_len, confidence=True,
                                                             packed=packed)
    frames, logp, post, score = frames.cpu().tolist(), logp.cpu().tolist(), post.cpu().tolist(), score.cpu().tolist()
    txt, n = txt.cpu().tolist(), [int(v) for v in txt_len.cpu().tolist()]
    return score, [token_rows(txt[u], n[u], frames[u], logp[u], post[u]) for u in range(len(n))]


def align_many(items, model, device):
    ''' several batch-1 loader items -> (name, score, token_rows) each, against the reference transcripts '''
    feat, lens = test_asr._pad_items(items, device)
    tl = [int((d[3][0] != 0).sum()) for d in items]
    txt = torch.zeros((len(items), max(max(tl), 1)), dtype=torch.int64)
    for u, d in enumerate(items):
        txt[u, :tl[u]] = d[3][0][d[3][0] != 0]
    score, rows = align_tokens(model, feat, lens, txt.to(device), torch.tensor(tl, device=device),
                               packed=len(items) > 1)
    return [(d[0][0], score[u], rows[u]) for u, d in enumerate(items)]


def align_hypotheses(model, feat, feat_len, hyps, device):
    ''' the best hypotheses (id lists) of the batch the search just ran on -> token_rows per utterance '''
    n = [len(h) for h in hyps]
    txt = torch.zeros((len(hyps), max(max(n), 1)), dtype=torch.int64)
    for u, h in enumerate(hyps):
        txt[u, :n[u]] = torch.tensor(h, dtype=torch.int64)
    return align_tokens(model, feat, feat_len, txt.to(device), torch.tensor(n, device=device))[1]


def write_rows(f, name, rows, tokenizer, sec):
    for pos, (tok, frame, logp, post) in enumerate(rows):
        f.write('\t'.join([name, str(pos), token_text(tokenizer, tok), str(frame), '{:.6f}'.format(frame * sec),
                           repr(float(logp)), repr(float(post))]) + '\n')


def write_times(times, path, tokenizer, sec):
    ''' [(name, token_rows)] -> the `_rnnt_times.tsv` file of one set '''
    with open(path, 'w', encoding='UTF-8') as f:
        f.write(TIMES_HEADER)
        for name, rows in times:
            write_rows(f, name, rows, tokenizer, sec)


def run(solver):
    ''' the `align: true` mode of bin/decode_asr.py's Solver (its loaders are instance-wise: batch size 1) '''
    group = max(1, int(os.environ.get('ASRK_DECODE_BATCH', '16')))
    if not solver.model.encoder.supports_packed():
        group = 1              # no packed encoder: padding would reach the recurrence
    sec = frame_seconds(solver)
    for s, ds in zip(['dev', 'test'], [solver.dv_set, solver.tt_set]):
        align_path = '{}_{}_rnnt_align.tsv'.format(solver.ckpdir, s)
        score_path = '{}_{}_rnnt_align_score.tsv'.format(solver.ckpdir, s)
        solver.verbose('Performing transducer forced alignment on {} set, num of utterances = {}.'.format(s, len(ds)))
        mine, ids, n_utt = solver._my_share(ds)
        local, pending = [], []
        for k, data in enumerate(mine):
            solver.progress('Align - {}/{}'.format(ids[k] + 1, n_utt))
            pending.append(data)
            if len(pending) == group:
                local += align_many(pending, solver.model, solver.device)
                pending = []
        if pending:
            local += align_many(pending, solver.model, solver.device)
        results = gather_in_order(local, n_utt, solver.dist, solver.rank, solver.world)
        if results is None:          # not rank 0: its rows have been handed over
            continue
        solver.verbose('Alignments / scores will be stored at {} / {}.'.format(align_path, score_path))
        with open(align_path, 'w', encoding='UTF-8') as fa, open(score_path, 'w') as fs:
            fa.write(TIMES_HEADER)
            fs.write(SCORE_HEADER)
            for name, score, rows in results:
                fs.write('{}\t{!r}\n'.format(name, float(score)))
                write_rows(fa, name, rows, solver.tokenizer, sec)
    solver.verbose('All done !')
