"""The testing solver `main.py --test` runs: bin/test_asr.py's Solver, with pure-CTC beam search WITH RNN-LM
fusion decoded in groups as well.

bin/test_asr.py decodes `ASRK_DECODE_BATCH` (default 16) utterances per `forward_batch` call of either decoder,
but sets the group to one for CTC + LM, from the time when that search went one launch + one LM step per frame
and utterance.  `CTCBeamDecoder.forward_batch` now advances the group in lock-step (one launch of U workgroups +
ONE LM step over all U x beam rows per frame: `search_device_batch`), so this solver hands it groups; everything
else - greedy decoding, the joint CTC-attention search, CTC search without an LM, output files, the fan-out over
ranks - is the parent class's.  `ASRK_DECODE_BATCH=1` still restores one utterance at a time.

A decode config with the reference's `emb:` block (`enable: true`, `fuse > 0`; reference: bin/test_asr.py:65-70) decodes
with embedding fusion: the plug-in (src/plugin.py) is built before the checkpoint is read, BaseSolver.load_ckpt fills it
from the checkpoint's `emb_decoder` entry, the parent hands it to the joint beam decoder, and for the greedy pass the model is
wrapped so that it is called with it; without the block nothing here changes.

The optional key `decode: {align: true}` turns the run into CTC forced alignment of both sets to their reference
transcripts instead of decoding (bin/align_asr.py); without the key nothing here changes.

The optional block `decode: {rescore: {enable: true, first_pass_lm: false, workspace_mb: 1024}}` selects two-pass
decoding (src/rescore.py): a CTC prefix beam search, then attention (+LM) rescoring of its n-best list.  The block
never reaches the other decoders; besides the usual two files (the beam file in rescored order) a third one,
`..._rescore-<beam>-<ctc_weight>-<lm_weight>.csv`, lists every hypothesis with its scores.  Without the block nothing
here changes.

The optional block `decode: {transducer: {enable: true, max_symbols: 3, max_len_ratio: 0.5}}` selects batched greedy
decoding with the RNN-transducer head (ASR.transducer_greedy; src/transducer.py) and writes the usual
`..._output.csv`; the block never reaches the beam decoders.  The training config must have built the head (`model:
transducer:`), otherwise the run stops with an error.  Without the block nothing here changes.
With `beam_size: W` (> 1) or `lm_weight` (> 0) in the block the hypotheses come from the transducer beam search
(ASR.transducer_beam: merged alignments, n-gram LM fusion from `decode.lm_path`, which must then be an ARPA / .ngram.npz
file); `..._output.csv` receives the best hypothesis and, with `nbest` > 1, `..._beam-<W>-<lm_weight>.csv` lists every
hypothesis with its score.  Otherwise the greedy search runs as before.
Two booleans of the block give token times (bin/align_rnnt.py): `align: true` turns the run into transducer forced
alignment of both sets to their reference transcripts (no search, no LM; `..._rnnt_align.tsv` and
`..._rnnt_align_score.tsv`), `timestamps: true` force-aligns the best hypothesis of the greedy or beam search and writes
`..._rnnt_times.tsv` beside the usual files, which stay byte for byte what they are without the key.

The optional block `decode: {bias: {path: PHRASES.txt | LIST.bias.npz, weight: 1.5}}` boosts a list of phrases in the
joint CTC-attention search, the CTC prefix search and the transducer beam search (src/bias.py: contextual biasing), alone
or fused with the n-gram LM of `decode.lm_path`; with `decode.transducer` it selects the beam search even at
`beam_size: 1`.  The block never reaches the beam decoders' keyword arguments.  It is refused at set-up with an RNN-LM,
with `rescore`, with transducer `align` and with greedy CTC / attention decoding.  Without the block nothing here changes.
"""
import os

from . import align_asr, align_rnnt, test_asr
from ..parallel import gather_in_order
from ..src.rescore import RescoreDecoder, check_decode_config
from ..src.transducer import take_decode_block, uses_beam
from ..src.bias import BiasedNGram, ContextBias, check_bias_config, install_bias, take_bias_block, tokenizer_encode


class _FusedGreedy:
    ''' the acoustic model as the greedy pass calls it, decoding over the plug-in's fused distribution '''

    def __init__(self, model, emb_decoder):
        self.model, self.emb_decoder = model, emb_decoder

    def __call__(self, feat, feat_len, decode_step):
        return self.model(feat, feat_len, decode_step, emb_decoder=self.emb_decoder)


class Solver(test_asr.Solver):
    ''' Solver for testing '''

    def __init__(self, config, paras, mode):
        self.align = bool(config['decode'].get('align', False))
        # taken out of the block like `rescore` below; enabled, the run takes the parent's greedy set-up (batch-wise
        # loaders, one output file per set), whatever decode.beam_size says: the transducer searches are batched and take
        # their own beam_size from the block
        self.transducer = take_decode_block(config['decode'])
        # contextual biasing (src/bias.py): taken out of the block as well; the combinations it excludes stop the run here
        self.bias_cfg = take_bias_block(config['decode'])
        check_bias_config(config['decode'], self.bias_cfg, transducer=self.transducer,
                          greedy=not self.transducer and not self.align and config['decode'].get('beam_size') == 1)
        if self.transducer:
            config['decode']['beam_size'] = 1       # (the parent's; the transducer's own is self.transducer['beam_size'])
            if self.bias_cfg:
                self.transducer['bias'] = True      # selects the beam search, as lm_weight > 0 does (uses_beam)
        check_decode_config(config['decode'], config.get('emb'))
        # taken out of the block: the parent hands the whole decode block to BeamDecoder(**dcfg)
        rescore = config['decode'].pop('rescore', None) or {}
        self.rescore = dict(rescore) if rescore.get('enable', False) else None
        if self.align:
            # the search settings are not used, but the parent reads beam_size: 1 makes it take its greedy set-up
            # (batch size of the training config) ...
            config['decode'].setdefault('beam_size', 1)
        super().__init__(config, paras, mode)
        if self.align or (self.transducer or {}).get('align', False):
            # ... which is replaced here by instance-wise loaders, like beam decoding.  This relies on the order
            # main.py keeps: load_data() builds the loaders from self.config AFTER __init__ has returned
            self.config['data']['corpus']['batch_size'] = 1

    def set_model(self):
        if getattr(self, 'transducer', None):
            init_adadelta = self.config['hparas']['optimizer'] == 'Adadelta'
            self.model = test_asr.ASR(self.feat_dim, self.vocab_size, init_adadelta,
                                      **self.config['model']).to(self.device)
            if not self.model.enable_rnnt:
                raise RuntimeError('decode.transducer needs a checkpoint with a transducer head: the training config '
                                   'has no enabled `model: transducer:` block')
            self.load_ckpt()        # eval mode
            self.decoder = self.model
            self.ctc_only = False
            self.enable_att = True  # (write_hyp: transducer hypotheses are never repeat-merged)
            self.transducer_lm = None
            if self.transducer.get('align', False):
                self.verbose(['Decode spec| Transducer forced alignment to the reference transcripts'])
                return
            if uses_beam(self.transducer):
                opts = self.transducer
                self.transducer_lm_weight = opts.get('lm_weight', 0.0)
                if opts.get('lm_weight', 0.0) > 0:
                    from ..src.ngram import NGramLM
                    self.transducer_lm = NGramLM.from_file(self.config['decode']['lm_path'],
                                                           self.vocab_size).to(self.device)
                bias = self.context_bias()
                if bias is not None and self.transducer_lm is not None:
                    self.transducer_lm = BiasedNGram.pair(self.transducer_lm, bias, opts['lm_weight'])
                elif bias is not None:
                    self.transducer_lm, self.transducer_lm_weight = bias, 1.0     # its rows are added as they are
                if bias is not None:
                    self.verbose(['Decode spec| Transducer beam search with contextual biasing']
                                 + self.transducer_lm.create_msg())
                self.verbose(['Decode spec| Transducer beam search \t| Beam size = {} | N-best = {} | LM weight = {} | '
                              'Max symbols per frame = {} | Max len ratio = {}'.format(
                                  opts.get('beam_size', 1), opts.get('nbest', 1), opts.get('lm_weight', 0.0),
                                  opts['max_symbols'], opts['max_len_ratio'])])
                return
            self.verbose(['Decode spec| Greedy transducer decoding \t| Max symbols per frame = {} | Max len ratio = {}'
                          .format(self.transducer['max_symbols'], self.transducer['max_len_ratio'])])
            return
        if getattr(self, 'rescore', None):
            init_adadelta = self.config['hparas']['optimizer'] == 'Adadelta'
            self.model = test_asr.ASR(self.feat_dim, self.vocab_size, init_adadelta,
                                      **self.config['model']).to(self.device)
            self.load_ckpt()        # eval mode
            dcfg = self.config['decode']
            self.decoder = RescoreDecoder(self.model, dcfg['beam_size'], dcfg['vocab_candidate'],
                                          ctc_weight=dcfg.get('ctc_weight', 0.0), lm_path=dcfg.get('lm_path', ''),
                                          lm_config=dcfg.get('lm_config', ''), lm_weight=dcfg.get('lm_weight', 0.0),
                                          first_pass_lm=self.rescore.get('first_pass_lm', False),
                                          workspace_mb=self.rescore.get('workspace_mb', 1024), device=self.device)
            self.ctc_only = False
            self.enable_att = self.model.enable_att
            self.verbose(self.decoder.create_msg())
            return
        if not getattr(self, 'align', False):
            super().set_model()
            if self.greedy and self.emb_decoder is not None:
                # the parent's greedy pass calls self.decoder(feat, feat_len, steps): the model, with the plug-in bound
                self.decoder = _FusedGreedy(self.model, self.emb_decoder)
            bias = self.context_bias()
            if bias is not None:
                # the parent built the beam decoder from the decode block, which no longer holds `bias`: the ContextBias
                # takes its scorer slot here (alone, or fused with the n-gram LM the parent loaded)
                install_bias(self.decoder, bias, self.device)
                self.verbose(self.decoder.lm.create_msg())
            return
        # alignment needs the acoustic model only: no search, no LM
        init_adadelta = self.config['hparas']['optimizer'] == 'Adadelta'
        self.model = test_asr.ASR(self.feat_dim, self.vocab_size, init_adadelta,
                                  **self.config['model']).to(self.device)
        self.load_ckpt()        # eval mode

    def context_bias(self):
        ''' the ContextBias of the `decode.bias` block (phrases encoded with the model's own text encoder), or None '''
        cfg = getattr(self, 'bias_cfg', None)
        if not cfg:
            return None
        return ContextBias.from_file(cfg['path'], self.vocab_size, weight=cfg['weight'],
                                     encode=tokenizer_encode(self.tokenizer)).to(self.device)

    def load_ckpt(self):
        ''' the parent's set_model calls this between building the model and building the decoder: the place where the
            plug-in has to exist (the checkpoint entry is loaded into it, the beam decoder is constructed with it) '''
        emb = self.config.get('emb')
        if emb and emb['enable'] and emb['fuse'] > 0 and not getattr(self, 'align', False):
            from ..src.plugin import EmbeddingRegularizer
            self.emb_decoder = EmbeddingRegularizer(self.tokenizer, self.model.dec_dim, **emb).to(self.device)
        super().load_ckpt()     # eval mode, plug-in included

    def greedy_decode(self, dv_set):
        ''' the parent's batch-wise pass; with decode.transducer the hypotheses come from ASR.transducer_greedy '''
        if not getattr(self, 'transducer', None):
            return super().greedy_decode(dv_set)
        results = []
        timestamps = self.transducer.get('timestamps', False)
        dv_set, batch_ids, _ = self._my_share(dv_set)
        for k, data in enumerate(dv_set):
            i = batch_ids[k]
            self.progress('Valid step - {}/{}'.format(i + 1, len(dv_set)))
            feat, feat_len, txt, txt_len = self.fetch_data(data)
            first = len(results)
            if uses_beam(self.transducer):
                opts = self.transducer
                tokens, n_tok, score, n_hyp, _ = self.model.transducer_beam(
                    feat, feat_len, opts.get('beam_size', 1), opts['max_symbols'], opts['max_len_ratio'],
                    nbest=opts.get('nbest', 1), lm=self.transducer_lm,
                    lm_weight=getattr(self, 'transducer_lm_weight', opts.get('lm_weight', 0.0)))
                tokens, n_tok, score, n_hyp = tokens.tolist(), n_tok.tolist(), score.tolist(), n_hyp.tolist()
                for j in range(len(txt)):
                    idx = j + self.config['data']['corpus']['batch_size'] * i
                    hyps = [tokens[j][h][:n_tok[j][h]] for h in range(n_hyp[j])]
                    if opts.get('nbest', 1) > 1:         # the scores travel with the hypotheses to write_hyp
                        hyps = [(hyp, score[j][h]) for h, hyp in enumerate(hyps)]
                    results.append((str(idx), hyps, txt[j].tolist()))
                if timestamps:
                    self._add_times(results, first, feat, feat_len)
                continue
            tokens, n_tok, _ = self.model.transducer_greedy(feat, feat_len, self.transducer['max_symbols'],
                                                            self.transducer['max_len_ratio'])
            tokens, n_tok = tokens.tolist(), n_tok.tolist()      # one read-back per batch, after the search
            for j in range(len(txt)):
                idx = j + self.config['data']['corpus']['batch_size'] * i
                results.append((str(idx), [tokens[j][:n_tok[j]]], txt[j].tolist()))
            if timestamps:
                self._add_times(results, first, feat, feat_len)
        return results

    def _add_times(self, results, first, feat, feat_len):
        ''' decode.transducer.timestamps: the rows results[first:] of the batch just searched get a fourth entry, the
            token times of their best hypothesis (write_hyp takes it off again before the usual files are written) '''
        best = [r[1][0] if r[1] else [] for r in results[first:]]
        best = [h[0] if isinstance(h, tuple) else h for h in best]       # (nbest > 1: the score travels with it)
        rows = align_rnnt.align_hypotheses(self.model, feat, feat_len, best, self.device)
        for k, r in enumerate(rows):
            results[first + k] = results[first + k] + (r,)

    def write_hyp(self, results, best_path, beam_path):
        ''' the parent's files; the n-best lists of the transducer beam search go to the beam file as well, one row per
            hypothesis with its score '''
        opts = getattr(self, 'transducer', None)
        if opts and opts.get('timestamps', False):
            tail = '_output.csv'
            assert best_path.endswith(tail)
            times_path = best_path[:-len(tail)] + '_rnnt_times.tsv'
            align_rnnt.write_times([(r[0], r[3]) for r in results], times_path, self.tokenizer,
                                   align_asr.frame_seconds(self))
            self.verbose('Token times of the hypotheses are stored at {}'.format(times_path))
            results = [r[:3] for r in results]
        if not (uses_beam(opts) and opts.get('nbest', 1) > 1):
            return super().write_hyp(results, best_path, beam_path)
        super().write_hyp([(name, [h[0] for h in hyps], truth) for name, hyps, truth in results], best_path, beam_path)
        tail = '_output.csv'
        assert best_path.endswith(tail)
        nbest_path = best_path[:-len(tail)] + '_beam-{}-{}.csv'.format(opts.get('beam_size', 1), opts.get('lm_weight', 0.0))
        with open(nbest_path, 'w', encoding='UTF-8') as f:
            f.write('idx\tbeam\tscore\thyp\ttruth\n')
            for name, hyps, truth in results:
                ref = self.tokenizer.decode(truth)
                for b, (hyp, score) in enumerate(hyps):
                    f.write('\t'.join([name, str(b), repr(score), self.tokenizer.decode(hyp), ref]) + '\n')
        self.verbose('N-best lists are stored at {}'.format(nbest_path))

    def exec(self):
        if getattr(self, 'align', False):      # (a solver assembled without __init__ decodes)
            return align_asr.run(self)
        if (getattr(self, 'transducer', None) or {}).get('align', False):
            return align_rnnt.run(self)
        if getattr(self, 'rescore', None):
            return self.exec_rescore()
        group = max(1, int(os.environ.get('ASRK_DECODE_BATCH', '16')))
        if self.greedy or not self.ctc_only or not self.decoder.apply_lm or group == 1:
            return super().exec()
        dcfg = self.config['decode']
        for s, ds in zip(['dev', 'test'], [self.dv_set, self.tt_set]):
            # files and messages as in the parent's beam branch (bin/test_asr.py: exec)
            self.cur_output_path = self.output_file.format(s, 'output')
            self.cur_beam_path = self.output_file.format(
                s, 'beam-{}-{}'.format(dcfg['beam_size'], dcfg.get('lm_weight', 0.0)))
            if self.rank == 0:
                with open(self.cur_output_path, 'w', encoding='UTF-8') as f:
                    f.write('idx\thyp\ttruth\n')
                with open(self.cur_beam_path, 'w') as f:
                    f.write('idx\tbeam\thyp\ttruth\n')
            self.verbose('Performing instance-wise CTC beam decoding on {} set, num of batch = {}.'.format(s, len(ds)))
            mine, ids, n_utt = self._my_share(ds)
            local, pending = [], []
            for k, data in enumerate(mine):
                self.progress('Decode - {}/{}'.format(ids[k] + 1, n_utt))
                pending.append(data)
                if len(pending) == group:
                    local += test_asr.ctc_beam_decode_many(pending, self.decoder, self.device)
                    pending = []
            if pending:
                local += test_asr.ctc_beam_decode_many(pending, self.decoder, self.device)
            results = gather_in_order(local, n_utt, self.dist, self.rank, self.world)
            if results is None:          # not rank 0: its rows have been handed over
                continue
            self.verbose('Results/Beams will be stored at {} / {}.'.format(self.cur_output_path, self.cur_beam_path))
            self.write_hyp(results, self.cur_output_path, self.cur_beam_path)
        self.verbose('All done !')

    def exec_rescore(self):
        ''' two-pass decoding: the parent's beam branch with RescoreDecoder.forward_batch per group, plus the score file '''
        dcfg = self.config['decode']
        group = max(1, int(os.environ.get('ASRK_DECODE_BATCH', '16')))
        for s, ds in zip(['dev', 'test'], [self.dv_set, self.tt_set]):
            self.cur_output_path = self.output_file.format(s, 'output')
            self.cur_beam_path = self.output_file.format(
                s, 'beam-{}-{}'.format(dcfg['beam_size'], dcfg.get('lm_weight', 0.0)))
            score_path = self.output_file.format(s, 'rescore-{}-{}-{}'.format(
                dcfg['beam_size'], dcfg.get('ctc_weight', 0.0), dcfg.get('lm_weight', 0.0)))
            if self.rank == 0:
                with open(self.cur_output_path, 'w', encoding='UTF-8') as f:
                    f.write('idx\thyp\ttruth\n')
                with open(self.cur_beam_path, 'w') as f:
                    f.write('idx\tbeam\thyp\ttruth\n')
                with open(score_path, 'w', encoding='UTF-8') as f:
                    f.write('idx\trank\tfirst_rank\tscore\tctc\tatt\tlm\thyp\ttruth\n')
            self.verbose('Performing CTC n-best rescoring on {} set, num of batch = {}.'.format(s, len(ds)))
            mine, ids, n_utt = self._my_share(ds)
            local, pending = [], []
            for k, data in enumerate(mine):
                self.progress('Decode - {}/{}'.format(ids[k] + 1, n_utt))
                pending.append(data)
                if len(pending) == group:
                    local += rescore_decode_many(pending, self.decoder, self.device)
                    pending = []
            if pending:
                local += rescore_decode_many(pending, self.decoder, self.device)
            results = gather_in_order(local, n_utt, self.dist, self.rank, self.world)
            if results is None:          # not rank 0: its rows have been handed over
                continue
            self.verbose('Results/Beams/Scores will be stored at {} / {} / {}.'.format(
                self.cur_output_path, self.cur_beam_path, score_path))
            self.write_hyp([(name, [list(h[0]) for h in hyps], truth) for name, hyps, truth in results],
                           self.cur_output_path, self.cur_beam_path)
            with open(score_path, 'a', encoding='UTF-8') as f:
                for name, hyps, truth in results:
                    ref = self.tokenizer.decode(truth)
                    for b, h in enumerate(hyps):
                        tokens, score, ctc, att, lm, first_rank = h
                        f.write('\t'.join([name, str(b), str(first_rank), repr(score), repr(ctc), repr(att), repr(lm),
                                           self.tokenizer.decode(list(tokens)), ref]) + '\n')
        self.verbose('All done !')


def rescore_decode_many(items, model, device):
    ''' several batch-1 loader items -> (name, [(tokens, score, ctc, att, lm, first_rank)] best first, truth) rows '''
    feat, lens = test_asr._pad_items(items, device)
    hyps = model.forward_batch(feat, lens)
    return [(d[0][0], [tuple(h) for h in hyps[u]], d[3][0].cpu().tolist()) for u, d in enumerate(items)]
