"""Training solver for hybrid CTC-attention ASR — mirror of the reference's bin/train_asr.py:9-247
(`Solver.fetch_data / load_data / set_model / exec / validate`, same step order: pre_step ->
forward -> CTC + CE losses -> backward -> clip -> step -> log -> validate -> checkpoint).

The model, both losses and the feature pipeline are the gfx950 kernels of this package; under
torch.distributed.run each rank takes its own shard of every epoch and gradients are averaged by
parallel.DataParallelEngine while BPTT is still running.
"""
import torch

from .. import ops
from ..src.solver import BaseSolver
from ..src.asr import ASR
from ..src.optim import Optimizer
from ..src.data import load_dataset
from ..src.audio import SpecAugment, SpeedPerturb, Dither, NoiseReverb
from ..src.loss import LossOptions
from ..src.mwer import MWEROptions, MWERLoss
from ..src.transducer import check_exclusive
from ..src.util import human_format, cal_er


class Solver(BaseSolver):
    ''' Solver for training'''

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.best_wer = {'att': 3.0, 'ctc': 3.0}
        # Curriculum learning affects data loader
        self.curriculum = self.config['hparas']['curriculum']

    def fetch_data(self, data):
        ''' batch is already resident in HBM (src/data.py); compute text seq. length '''
        _, feat, feat_len, txt = data
        # transcripts arrive on the host: their lengths (and the number of decoder steps, the longest of them) are
        # computed THERE - reading `int(txt_len.max())` back from the device would stall the host on the previous
        # step's kernels once per step
        txt_len = torch.sum(txt != 0, dim=-1)
        self.decode_step = int(txt_len.max())
        feat = feat.to(self.device)
        feat_len = feat_len.to(self.device)
        txt = txt.to(self.device)
        txt_len = txt_len.to(self.device)
        return feat, feat_len, txt, txt_len

    def load_data(self):
        # waveform augmentation of the training loader (top-level `speed_perturb:` block; None = every batch is exactly
        # what it was); drawn per (seed, epoch, utterance name): see exec()
        self.speed = SpeedPerturb.from_config(self.config, seed=self.paras.seed)
        # the filterbank's dither (data.audio.dither; None = 0 or absent: no launch changes): one key per utterance,
        # per epoch for the training loader, fixed for the dev loader
        self.dither = Dither.from_config(self.config, seed=self.paras.seed)
        # reverberation and additive noise of the training loader (top-level `noise_reverb:` block; None = no launch
        # changes); drawn per (seed, epoch, utterance name) like the speed factors; never applied to the dev loader
        self.noise_reverb = NoiseReverb.from_config(self.config, seed=self.paras.seed)
        self.tr_set, self.dv_set, self.feat_dim, self.vocab_size, self.tokenizer, msg = \
            load_dataset(self.paras.njobs, self.paras.gpu, self.paras.pin_memory,
                         self.curriculum > 0, speed_perturb=self.speed, dither=self.dither,
                         noise_reverb=self.noise_reverb, **self.config['data'])
        self.verbose(msg)
        if self.speed is not None:
            self.verbose(self.speed.create_msg())
        if self.dither is not None:
            self.verbose(self.dither.create_msg())
        if self.noise_reverb is not None:
            self.verbose(self.noise_reverb.create_msg())
        # training-time input augmentation (top-level `specaug:` block; None = the step is exactly what it was)
        audio = self.config['data']['audio']
        self.specaug = SpecAugment.from_config(self.config, audio['feat_dim'], audio.get('delta_order', 0) + 1)
        if self.specaug is not None:
            self.verbose(self.specaug.create_msg())

    def set_model(self):
        ''' Setup ASR model and optimizer '''
        init_adadelta = self.config['hparas']['optimizer'] == 'Adadelta'
        check_exclusive(self.config)         # `model: transducer:` beside `mwer:` or `emb:` is refused
        self.model = ASR(self.feat_dim, self.vocab_size, init_adadelta, **self.config['model']).to(self.device)
        self.verbose(self.model.create_msg())
        model_paras = [{'params': self.model.parameters()}]
        # Losses (gfx950 kernels behind the torch.nn loss-module surface)
        # (top-level `loss:` block; absent = plain cross entropy and zero_infinity=False, as ever)
        opts = LossOptions.from_config(self.config)
        self.seq_loss = ops.CrossEntropyLoss(ignore_index=0, label_smoothing=opts.label_smoothing)
        self.ctc_loss = ops.CTCLoss(blank=0, zero_infinity=opts.ctc_zero_infinity)
        # transducer head (`model: transducer:` block; absent or disabled = the step is exactly what it was)
        self.rnnt_on = self.model.enable_rnnt
        if self.rnnt_on:
            self.rnnt_loss = ops.RNNTLoss(blank=0)
            self.best_wer['rnnt'] = 3.0
            dec = (self.config.get('decode') or {}).get('transducer') or {}
            self.rnnt_max_symbols = int(dec.get('max_symbols', 3))
            self.rnnt_max_len_ratio = float(dec.get('max_len_ratio', 0.5))
        if opts.active:
            self.verbose(opts.create_msg())
        # Plug-ins (reference: bin/train_asr.py:51-63): word-embedding regulariser / embedding-fusion decoder
        self.emb_fuse = False
        self.emb_reg = ('emb' in self.config) and bool(self.config['emb']['enable'])
        if self.emb_reg:
            if self.world > 1:
                raise NotImplementedError(
                    'emb.enable with WORLD_SIZE > 1: the data-parallel engine averages the gradients of the model '
                    'only, the plug-in\'s parameters would drift apart between ranks; train it on one GPU')
            from ..src.plugin import EmbeddingRegularizer
            self.emb_decoder = EmbeddingRegularizer(
                self.tokenizer, self.model.dec_dim, **self.config['emb']).to(self.device)
            model_paras.append({'params': self.emb_decoder.parameters()})
            self.emb_fuse = self.emb_decoder.apply_fuse
            if self.emb_fuse:
                if opts.label_smoothing != 0.0:
                    raise ValueError('loss.label_smoothing with emb.fuse: smoothing is defined on logits, the fused '
                                     'decoder output is a log-probability; drop one of the two')
                self.seq_loss = ops.NLLLoss(ignore_index=0)
            self.verbose(self.emb_decoder.create_msg())
        self.optimizer = Optimizer(model_paras, **self.config['hparas'])
        self.verbose(self.optimizer.create_msg())
        # MWER fine-tuning (top-level `mwer:` block; None = the step is exactly what it was)
        self.mwer = None
        mwer_opts = MWEROptions.from_config(self.config)
        if mwer_opts is not None:
            self.mwer = MWERLoss(self.model, self.tokenizer, mwer_opts)
            self.verbose(self.mwer.create_msg())
        self.load_ckpt()
        self.enable_data_parallel()

    def compute_losses(self, ctc_output, encode_len, att_output, txt, txt_len, emb_loss=None):
        ''' (reference: bin/train_asr.py:108-133) -> (loss to back-propagate, ctc_loss, att_loss, total loss as the
            reference would log it for this rank's batch).  `att_output` is the fused log-probability under embedding
            fusion (seq_loss is then the NLL loss); `emb_loss` enters with the plug-in's weight.

            Data parallel (one process per GPU, gradients AVERAGED over ranks by parallel.DataParallelEngine): for the
            update to equal the single-process step on the GLOBAL batch (SURVEY §8e cond. 1, 2)
              * CTCLoss 'mean' = mean over utterances of nll_b / len_b  -> weight B_rank / (B_global / world);
              * CrossEntropy(ignore_index=0) 'mean' = mean over non-pad tokens -> weight N_rank / (N_global / world).
            Both counts travel in ONE scalar all-reduce; the logged losses stay the rank's own unweighted ones. '''
        total_loss, shown_loss, ctc_loss, att_loss = 0, 0, None, None
        w_ctc = w_att = None
        if self.dp is not None:
            counts = torch.stack([txt_len.new_tensor(txt.shape[0]), txt_len.sum()]).to(torch.float64)
            w = (counts / self.dp.count_normaliser(counts)).to(torch.float32)
            w_ctc, w_att = w[0], w[1]
        self.w_utt = w_ctc          # the utterance-count weight of this step (MWER is a mean over utterances too)
        if emb_loss is not None:
            shown_loss = shown_loss + emb_loss.detach() * self.emb_decoder.weight
            total_loss += emb_loss * self.emb_decoder.weight
        if ctc_output is not None:
            ctc_loss = self.ctc_loss(ctc_output.transpose(0, 1), txt, encode_len, txt_len)
            shown_loss = shown_loss + ctc_loss.detach() * self.model.ctc_weight
            total_loss += (ctc_loss if w_ctc is None else ctc_loss * w_ctc) * self.model.ctc_weight
        if att_output is not None:
            b, t, _ = att_output.shape
            att_loss = self.seq_loss(att_output.view(b * t, -1), txt.view(-1))
            shown_loss = shown_loss + att_loss.detach() * (1 - self.model.ctc_weight)
            total_loss += (att_loss if w_att is None else att_loss * w_att) * (1 - self.model.ctc_weight)
        return total_loss, ctc_loss, att_loss, shown_loss

    def exec(self):
        ''' Training End-to-end ASR system '''
        self.verbose('Total training steps {}.'.format(human_format(self.max_step)))
        ctc_loss, att_loss, emb_loss, rnnt_loss = None, None, None, None
        rnnt_pruned, rnnt_simple = None, None
        n_epochs = 0
        self.timer.set()
        while self.step < self.max_step:
            # Renew dataloader to enable random sampling
            if self.curriculum > 0 and n_epochs == self.curriculum:
                self.verbose('Curriculum learning ends after {} epochs, starting random sampling.'.format(n_epochs))
                self.tr_set, _, _, _, _, _ = load_dataset(self.paras.njobs, self.paras.gpu,
                                                          self.paras.pin_memory, False, speed_perturb=self.speed,
                                                          dither=self.dither, noise_reverb=self.noise_reverb,
                                                          **self.config['data'])
            if hasattr(self.tr_set.sampler, 'set_epoch'):     # data parallel: the shared shuffle of this epoch
                self.tr_set.sampler.set_epoch(n_epochs)
            if self.speed is not None:
                # this epoch's speed factors are keyed by the step it starts at (a run resumed in mid-epoch draws the
                # rest of that epoch from the step it resumed at)
                self.speed.begin_epoch(self.step)
            if self.dither is not None:
                self.dither.begin_epoch(self.step)             # the same epoch key as the speed factors'
            if self.noise_reverb is not None:
                self.noise_reverb.begin_epoch(self.step)
            for data in self.tr_set:
                # Pre-step : update tf_rate/lr_rate and do zero_grad
                tf_rate = self.optimizer.pre_step(self.step)
                feat, feat_len, txt, txt_len = self.fetch_data(data)
                if self.specaug is not None:
                    # keyed by (seed, step, rank): a resumed run continues the same stream; data[2] = the lengths
                    # on the host, as the collate function made them (no read-back)
                    feat = self.specaug(feat, data[2], self.paras.seed, self.step, self.rank, feat_len_dev=feat_len)
                self.timer.cnt('rd')

                # MWER step: the n-best lists of this batch first (the search runs its own eval-mode encoder pass)
                mwer_on = self.mwer is not None and self.step >= self.mwer.opts.start_step
                nbest = self.mwer.nbest(feat, feat_len) if mwer_on else None
                # the MWER step runs the encoder itself: the hypotheses are scored on the very output the training
                # forward decodes from (ASR.forward(encoded=...): the same call it would make, so the same launches)
                # (so does the transducer step: its head reads the encoder output the CTC head reads)
                encoded = self.model.encoder(feat, feat_len) if (mwer_on or self.rnnt_on) else None

                # Note: txt should NOT start w/ <sos>
                if not self.emb_reg:
                    if encoded is not None:
                        ctc_output, encode_len, att_output, att_align, dec_state = \
                            self.model(feat, feat_len, self.decode_step, tf_rate=tf_rate, teacher=txt, encoded=encoded)
                    else:
                        ctc_output, encode_len, att_output, att_align, dec_state = \
                            self.model(feat, feat_len, self.decode_step, tf_rate=tf_rate, teacher=txt)
                    total_loss, ctc_loss, att_loss, shown_loss = \
                        self.compute_losses(ctc_output, encode_len, att_output, txt, txt_len)
                    if mwer_on:
                        # data[3]: the transcripts on the host, as the collate function made them (no read-back)
                        mwer_loss, mwer_stats = self.mwer(nbest, encoded[0], encode_len, data[3])
                        mwer_loss = mwer_loss.to(torch.float32)
                        ce_w = self.mwer.opts.ce_weight
                        shown_loss = mwer_loss.detach() + ce_w * shown_loss
                        total_loss = (mwer_loss if self.w_utt is None else mwer_loss * self.w_utt) + ce_w * total_loss
                    if self.rnnt_on:
                        # a mean over utterances like CTC: the utterance-count weight under data parallel.  The loss's
                        # backward writes the gradient over the logits (nothing else reads them)
                        if self.model.rnnt_prune is not None:
                            # pruned training: the band loss plus simple_weight times the simple joiner's
                            rnnt_loss, rnnt_pruned, rnnt_simple = \
                                self.model.transducer_loss_pruned(encoded[0], encode_len, txt, txt_len)
                        else:
                            logits = self.model.transducer_logits(encoded[0], encode_len, txt, txt_len)
                            rnnt_loss = self.rnnt_loss(logits, txt, encode_len, txt_len, consume_logits=True)
                            del logits
                        shown_loss = shown_loss + rnnt_loss.detach() * self.model.rnnt_weight
                        total_loss = total_loss + \
                            (rnnt_loss if self.w_utt is None else rnnt_loss * self.w_utt) * self.model.rnnt_weight
                else:
                    ctc_output, encode_len, att_output, att_align, dec_state = \
                        self.model(feat, feat_len, self.decode_step, tf_rate=tf_rate, teacher=txt, get_dec_state=True)
                    emb_loss, fuse_output = self.emb_decoder(dec_state, att_output, label=txt)
                    if self.emb_fuse:
                        att_output = fuse_output        # the attention loss and the error rate read the mixture
                    total_loss, ctc_loss, att_loss, shown_loss = \
                        self.compute_losses(ctc_output, encode_len, att_output, txt, txt_len, emb_loss=emb_loss)
                self.timer.cnt('fw')

                grad_norm = self.backward(total_loss)
                self.step += 1
                self.poll_device_errors()

                if (self.step == 1) or (self.step % self.PROGRESS_STEP == 0):
                    self.progress('Tr stat | Loss - {:.2f} | Grad. Norm - {:.2f} | {}'
                                  .format(shown_loss.detach().cpu().item(), float(grad_norm), self.timer.show()))
                    self.write_log('loss', {'tr_ctc': ctc_loss, 'tr_att': att_loss, 'tr_rnnt': rnnt_loss,
                                            'tr_rnnt_pruned': rnnt_pruned, 'tr_rnnt_simple': rnnt_simple})
                    if mwer_on:
                        self.write_log('mwer', {'tr_exp_err': mwer_stats['exp_err'],
                                                'tr_1best_err': mwer_stats['best_err']})
                    if self.emb_reg:
                        self.write_log('emb_loss', {'tr': emb_loss})
                        if self.emb_fuse:
                            if self.emb_decoder.fuse_learnable:
                                self.write_log('fuse_lambda', {'emb': self.emb_decoder.get_weight()})
                            self.write_log('fuse_temp', {'temp': self.emb_decoder.get_temp()})
                    # zero_infinity: utterances of this step whose transcript did not fit their encoder frames
                    # (getattr: a torch loss module has no such counter)
                    n_zeroed = getattr(self.ctc_loss, 'n_infeasible', None)
                    n_zeroed = int(n_zeroed) if n_zeroed is not None and ctc_loss is not None else 0
                    if n_zeroed:
                        self.verbose('CTC zero_infinity : {} utterance(s) zeroed @ step {}'.format(n_zeroed, self.step))
                        self.write_log('ctc_zeroed', {'tr': n_zeroed})
                    self.write_log('wer', {'tr_att': cal_er(self.tokenizer, att_output, txt),
                                           'tr_ctc': cal_er(self.tokenizer, ctc_output, txt, ctc=True)})

                if (self.step == 1) or (self.step % self.valid_step == 0):
                    self.validate()

                self.timer.set()
                if self.step > self.max_step:
                    break
            n_epochs += 1
        self.poll_device_errors(force=True)
        if self.log is not None:
            self.log.close()

    def validate(self):
        with self.averaged_weights():           # hparas.average: scores and checkpoints of the averaged weights
            self._validate()

    def _validate(self):
        self.poll_device_errors(force=True)     # a validation score / checkpoint of parameters that are known good
        self.model.eval()
        if self.emb_decoder is not None:
            self.emb_decoder.eval()
        dev_wer = {'att': [], 'ctc': []}
        if self.rnnt_on:
            dev_wer['rnnt'] = []
        for i, data in enumerate(self.dv_set):
            self.progress('Valid step - {}/{}'.format(i + 1, len(self.dv_set)))
            feat, feat_len, txt, txt_len = self.fetch_data(data)
            with torch.no_grad():
                if not self.emb_fuse:   # (a regulariser-only plug-in has no say in decoding: the fused greedy loop)
                    ctc_output, encode_len, att_output, att_align, dec_state = \
                        self.model(feat, feat_len, int(self.decode_step * self.DEV_STEP_RATIO))
                else:       # greedy decoding over the fused distribution: the per-step loop of ASR.forward
                    ctc_output, encode_len, att_output, att_align, dec_state = \
                        self.model(feat, feat_len, int(self.decode_step * self.DEV_STEP_RATIO),
                                   emb_decoder=self.emb_decoder)
            dev_wer['att'].append(cal_er(self.tokenizer, att_output, txt))
            dev_wer['ctc'].append(cal_er(self.tokenizer, ctc_output, txt, ctc=True))
            if self.rnnt_on:
                with torch.no_grad():
                    rnnt_tok, _, _ = self.model.transducer_greedy(feat, feat_len, self.rnnt_max_symbols,
                                                                  self.rnnt_max_len_ratio)
                dev_wer['rnnt'].append(cal_er(self.tokenizer, rnnt_tok, txt))

            # Log some examples
            if i == len(self.dv_set) // 2:
                for j in range(min(len(txt), self.DEV_N_EXAMPLE)):
                    if self.step == 1:
                        self.write_log('true_text{}'.format(j), self.tokenizer.decode(txt[j].tolist()))
                    if att_output is not None:
                        self.write_log('att_text{}'.format(j), self.tokenizer.decode(
                            ops.argmax(att_output[j]).tolist()))
                    if ctc_output is not None:
                        self.write_log('ctc_text{}'.format(j), self.tokenizer.decode(
                            ops.argmax(ctc_output[j]).tolist(), ignore_repeat=True))

        # Ckpt if performance improves
        for task in list(dev_wer):
            dev_wer[task] = sum(dev_wer[task]) / len(dev_wer[task])
            if dev_wer[task] < self.best_wer[task]:
                self.best_wer[task] = dev_wer[task]
                self.save_checkpoint('best_{}.pth'.format(task), 'wer', dev_wer[task])
            self.write_log('wer', {'dv_' + task: dev_wer[task]})
        self.save_checkpoint('latest.pth', 'wer', dev_wer['att'], show_msg=False)
        self.model.train()
        if self.emb_decoder is not None:
            self.emb_decoder.train()
