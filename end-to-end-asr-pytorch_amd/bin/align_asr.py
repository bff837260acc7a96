"""`main.py --test` with `decode: {align: true}`: CTC forced alignment of the dev and test sets.

Every utterance is aligned to its REFERENCE transcript with the model's CTC head (ASR.ctc_align: the best CTC
path, found and traced back on the device - csrc/ctc.hip).  Utterances go through in groups of `ASRK_DECODE_BATCH`
(default 16), through the packed encoder where the model has one (every utterance encoded as if alone, so grouping and
padding never change an alignment; else one utterance at a time), and fan out over ranks like the decoding modes
(bin/test_asr.py: _my_share / gather_in_order).  Rank 0 writes, per set,

    <outdir>/<name>_{dev,test}_align.tsv        idx, pos, token, start_frame, end_frame, start_s, end_s
                                                one row per target token; frames are ENCODER frames, end exclusive
    <outdir>/<name>_{dev,test}_align_score.tsv  idx, score: log-probability of the best path (-inf: the transcript
                                                does not fit the utterance's frames; it then has no token rows)

seconds = frame x encoder subsampling x feature frame shift: what the encoder and the feature transform built from the
training config answer for.
"""
import os

import torch

from . import test_asr
from ..parallel import gather_in_order

ALIGN_HEADER = 'idx\tpos\ttoken\tstart_frame\tend_frame\tstart_s\tend_s\n'
SCORE_HEADER = 'idx\tscore\n'


def frame_seconds(solver):
    ''' seconds per encoder frame: the encoder's own subsampling (prenet and every layer's sample_rate, as
        Encoder.__init__ derives it from the model config) times the feature transform's frame shift (the audio
        config's, as the loaders' transform holds it) '''
    transform = solver.dv_set.collate_fn.keywords['audio_transform']
    return solver.model.encoder.sample_rate * transform[0].frame_shift_ms() * 0.001


def token_text(tokenizer, idx):
    if hasattr(tokenizer, 'idx_to_vocab'):
        return tokenizer.idx_to_vocab(idx)
    if hasattr(tokenizer, 'spm'):
        return tokenizer.spm.id_to_piece(int(idx))
    return str(idx)


def align_many(items, model, device):
    ''' several batch-1 loader items -> (name, score, [(token id, first frame, last frame + 1), ...]) each '''
    feat, lens = test_asr._pad_items(items, device)
    tl = [int((d[3][0] != 0).sum()) for d in items]
    txt = torch.zeros((len(items), max(max(tl), 1)), dtype=torch.int64)
    for u, d in enumerate(items):
        txt[u, :tl[u]] = d[3][0][d[3][0] != 0]
    txt = txt.to(device)
    _, _, spans, score, _ = model.ctc_align(feat, lens, txt, torch.tensor(tl, device=device), packed=len(items) > 1)
    spans, score, txt = spans.cpu().tolist(), score.cpu().tolist(), txt.cpu().tolist()
    out = []
    for u, d in enumerate(items):
        rows = [(txt[u][l], spans[u][l][0], spans[u][l][1]) for l in range(tl[u]) if spans[u][l][0] >= 0]
        out.append((d[0][0], score[u], rows))
    return out


def write_alignments(results, align_path, score_path, tokenizer, sec):
    with open(align_path, 'a', encoding='UTF-8') as fa, open(score_path, 'a') as fs:
        for name, score, rows in results:
            fs.write('{}\t{!r}\n'.format(name, float(score)))
            for pos, (tok, t0, t1) in enumerate(rows):
                fa.write('\t'.join([name, str(pos), token_text(tokenizer, tok), str(t0), str(t1),
                                    '{:.6f}'.format(t0 * sec), '{:.6f}'.format(t1 * sec)]) + '\n')


def run(solver):
    ''' the alignment mode of bin/decode_asr.py's Solver (its loaders are instance-wise: batch size 1) '''
    if not solver.model.enable_ctc:
        raise RuntimeError('decode.align needs a model with a CTC head (ctc_weight > 0)')
    group = max(1, int(os.environ.get('ASRK_DECODE_BATCH', '16')))
    if not solver.model.encoder.supports_packed():
        group = 1              # no packed encoder: padding would reach the recurrence
    sec = frame_seconds(solver)
    for s, ds in zip(['dev', 'test'], [solver.dv_set, solver.tt_set]):
        align_path = '{}_{}_align.tsv'.format(solver.ckpdir, s)
        score_path = '{}_{}_align_score.tsv'.format(solver.ckpdir, s)
        if solver.rank == 0:
            with open(align_path, 'w', encoding='UTF-8') as f:
                f.write(ALIGN_HEADER)
            with open(score_path, 'w') as f:
                f.write(SCORE_HEADER)
        solver.verbose('Performing CTC forced alignment on {} set, num of utterances = {}.'.format(s, len(ds)))
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
        write_alignments(results, align_path, score_path, solver.tokenizer, sec)
    solver.verbose('All done !')
