"""ASR model (Listener / Attention / Speller + CTC head) — MI355X mirror of the reference's
src/asr.py: same class names, constructor kwargs, attributes, state_dict keys and return tuple.
"""
import numpy as np
import torch
import torch.nn as nn
from torch.distributions.categorical import Categorical

from .. import ops
from .. import decoder_ops as dops
from .. import speller_ops as sops
from .util import init_weights, init_gate
from .transducer import TransducerHead, transducer_enabled, take_prune_block
from .module import (VGGExtractor, CNNExtractor, RNNLayer, RNNParams, ScaleDotAttention,
                     LocationAwareAttention)


SCORE_BLOCK = 16     # hypotheses per launch group of ASR.score_hypotheses (fixed: see there)


class ASR(nn.Module):
    ''' ASR model, including Encoder/Decoder(s) (reference: src/asr.py:12-155) '''

    def __init__(self, input_size, vocab_size, init_adadelta, ctc_weight, encoder, attention,
                 decoder, emb_drop=0.0, transducer=None):
        super(ASR, self).__init__()

        assert 0 <= ctc_weight <= 1
        self.vocab_size = vocab_size
        self.ctc_weight = ctc_weight
        self.enable_ctc = ctc_weight > 0
        self.enable_att = ctc_weight != 1
        self.lm = None

        self.encoder = Encoder(input_size, **encoder)
        if self.enable_ctc:
            self.ctc_layer = nn.Linear(self.encoder.out_dim, vocab_size)
        if self.enable_att:
            self.dec_dim = decoder['dim']
            self.pre_embed = nn.Embedding(vocab_size, self.dec_dim)
            self.embed_drop = nn.Dropout(emb_drop)
            self.decoder = Decoder(self.encoder.out_dim + self.dec_dim, vocab_size, **decoder)
            query_dim = self.dec_dim * self.decoder.layer
            self.attention = Attention(self.encoder.out_dim, query_dim, **attention)
        # RNN-transducer head (the `model: transducer:` block; absent or enable: false = no new parameter, no new key)
        self.enable_rnnt = transducer_enabled(transducer)
        self.rnnt_weight = 0.0
        self.rnnt_prune = None
        if self.enable_rnnt:
            unknown = sorted(set(transducer) - {'enable', 'weight', 'joint_dim', 'pred', 'prune'}, key=str)
            if unknown:
                raise ValueError('model.transducer: unknown key(s) {}'.format(unknown))
            self.rnnt_weight = float(transducer.get('weight', 0.3))
            # pruned training (the `prune:` sub-block; absent or enable: false = no new parameter, no new key)
            self.rnnt_prune = take_prune_block(transducer.get('prune'))
            self.transducer = TransducerHead(vocab_size, self.encoder.out_dim, dict(transducer.get('pred') or {}),
                                             int(transducer.get('joint_dim', 512)), prune=self.rnnt_prune)

        if init_adadelta:
            self.apply(init_weights)
            if self.enable_att:
                for l in range(self.decoder.layer):
                    bias = getattr(self.decoder.layers, 'bias_ih_l{}'.format(l))
                    bias = init_gate(bias)

    def set_state(self, prev_state, prev_attn):
        ''' Setting up all memory states for beam decoding'''
        self.decoder.set_state(prev_state)
        self.attention.set_mem(prev_attn)

    def create_msg(self):
        msg = []
        msg.append('Model spec.| Encoder\'s downsampling rate of time axis is {}.'.format(
            self.encoder.sample_rate))
        if self.encoder.vgg:
            msg.append('           | VGG Extractor w/ time downsampling rate = 4 in encoder enabled.')
        if self.encoder.cnn:
            msg.append('           | CNN Extractor w/ time downsampling rate = 4 in encoder enabled.')
        if self.enable_ctc:
            msg.append('           | CTC training on encoder enabled ( lambda = {}).'.format(
                self.ctc_weight))
        if self.enable_att:
            msg.append('           | {} attention decoder enabled ( lambda = {}).'.format(
                self.attention.mode, 1 - self.ctc_weight))
        if self.enable_rnnt:
            msg.append(self.transducer.create_msg())
        return msg

    def _need_transducer(self, what):
        if not self.enable_rnnt:
            raise RuntimeError('ASR.{} needs a transducer head: this model was built without the '
                               '`model: transducer:` block'.format(what))

    def transducer_logits(self, encode_feature, encode_len, txt, txt_len):
        ''' joint logits [B,T',U+1,V] of the transducer head on the encoder's output (of the training forward:
            ASR.forward(encoded=...)), for ops.RNNTLoss(consume_logits=True); txt [B,L] padded labels, txt_len [B] '''
        self._need_transducer('transducer_logits')
        return self.transducer(encode_feature, encode_len, txt, txt_len)

    def transducer_loss_pruned(self, encode_feature, encode_len, txt, txt_len):
        ''' the pruned transducer training loss on the encoder's output (`model: transducer: prune:`) ->
            (pruned_nll + simple_weight * simple_nll, pruned_nll, simple_nll), means over the utterances; the head's
            weight is the caller's (TransducerHead.forward_pruned) '''
        self._need_transducer('transducer_loss_pruned')
        if self.rnnt_prune is None:
            raise RuntimeError('ASR.transducer_loss_pruned needs the `model: transducer: prune:` block')
        pruned, simple = self.transducer.forward_pruned(encode_feature, encode_len, txt, txt_len)
        return pruned + self.rnnt_prune['simple_weight'] * simple, pruned, simple

    @torch.no_grad()
    def transducer_greedy(self, audio_feature, feature_len, max_symbols=3, max_len_ratio=0.5):
        ''' batched greedy transducer decoding: encoder -> TransducerHead.greedy with at most max_symbols tokens per
            encoder frame and ceil(max_len_ratio * T') tokens per utterance.
            Returns (tokens int64 [B, max_len] zero-padded, n_tokens int32 [B], encode_len [B]), all on the device '''
        self._need_transducer('transducer_greedy')
        encode_feature, encode_len = self.encoder(audio_feature, feature_len)
        max_len = max(1, int(np.ceil(encode_feature.shape[1] * float(max_len_ratio))))
        tokens, n_tok = self.transducer.greedy(encode_feature, encode_len, max_symbols, max_len)
        return tokens, n_tok, encode_len

    @torch.no_grad()
    def transducer_beam(self, audio_feature, feature_len, beam_size, max_symbols=3, max_len_ratio=0.5, nbest=1, lm=None,
                        lm_weight=0.0):
        ''' batched transducer beam search with merged alignments and optional n-gram LM fusion: encoder ->
            TransducerHead.beam_search, the limits as in transducer_greedy.  Returns (tokens int64 [B, nbest, max_len]
            zero-padded, n_tokens int32 [B, nbest], score float64 [B, nbest], n_hyp int32 [B], encode_len [B]), best
            hypothesis first, all on the device '''
        self._need_transducer('transducer_beam')
        encode_feature, encode_len = self.encoder(audio_feature, feature_len)
        max_len = max(1, int(np.ceil(encode_feature.shape[1] * float(max_len_ratio))))
        tokens, n_tok, score, n_hyp = self.transducer.beam_search(encode_feature, encode_len, beam_size, max_symbols,
                                                                  max_len, nbest=nbest, lm=lm, lm_weight=lm_weight)
        return tokens, n_tok, score, n_hyp, encode_len

    @torch.no_grad()
    def transducer_align(self, audio_feature, feature_len, txt, txt_len, confidence=False, max_logits_bytes=1 << 30,
                         packed=False):
        ''' Forced alignment of every utterance to its transcript with the transducer head: encoder ->
            TransducerHead.lattice_logp (at most max_logits_bytes of joint logits at a time) -> optionally the alpha /
            beta lattice -> ops.rnnt_align (the best path, found and traced back on the device).  txt [B,U] padded
            token ids, txt_len [B].  Returns (frames [B,U], labels_done [B,T'], tok_logp [B,U], tok_post [B,U] or None
            without confidence, score [B], encode_len [B]): frames are ENCODER frames; tokens >= txt_len[b] and frames
            >= encode_len[b] hold -1; a score of -inf means the transcript does not fit.  packed=True (needs
            encoder.supports_packed()): every utterance is encoded as if alone and unpadded, as in ctc_align. '''
        self._need_transducer('transducer_align')
        encode_feature, encode_len = self.encoder(audio_feature, feature_len, packed=packed)
        al = self.transducer.align(encode_feature, encode_len, txt, txt_len, confidence=confidence,
                                   max_logits_bytes=max_logits_bytes)
        return al.frames, al.labels_done, al.tok_logp, al.tok_post, al.score, encode_len

    @torch.no_grad()
    def ctc_align(self, audio_feature, feature_len, txt, txt_len, packed=False):
        ''' Forced alignment of every utterance to its transcript with the CTC head: encoder -> CTC head ->
            log_softmax -> ops.ctc_align (the best CTC path, found and traced back on the device).  txt [B,L] padded
            token ids, txt_len [B].  Returns (states [B,T'], tokens [B,T'], spans [B,L,2], score [B], encode_len [B]):
            frames are ENCODER frames (see ops.ctc_align); frames >= encode_len[b] and tokens >= txt_len[b] hold -1.
            packed=True (needs encoder.supports_packed()): every utterance is encoded as if alone and unpadded, so
            the other utterances of the batch and its padding never change an alignment. '''
        if not self.enable_ctc:
            raise RuntimeError('ASR.ctc_align needs a CTC head: this model was built with ctc_weight = 0')
        encode_feature, encode_len = self.encoder(audio_feature, feature_len, packed=packed)
        ctc_output = ops.log_softmax(ops.linear(encode_feature, self.ctc_layer.weight, self.ctc_layer.bias))
        # the [T',B,V] view of the [B,T',V] log-probs: the kernel takes the strides, nothing is copied
        al = ops.ctc_align(ctc_output.transpose(0, 1), txt, encode_len, txt_len, blank=0)
        return al.states, al.tokens, al.spans, al.score, encode_len

    def forward(self, audio_feature, feature_len, decode_step, tf_rate=0.0, teacher=None,
                emb_decoder=None, get_dec_state=False, encoded=None):
        ''' Same contract as the reference (src/asr.py:72-155): returns
            (ctc_output [B,T',V] log-probs | None, encode_len [B], att_output [B,L,V] logits | None,
             att_seq [B,N,L,T'] | None, dec_state [B,L,D] | None) '''
        bs = audio_feature.shape[0]
        ctc_output, att_output, att_seq = None, None, None
        dec_state = [] if get_dec_state else None

        # encoded: (encode_feature, encode_len) of self.encoder(audio_feature, feature_len), when the caller ran the
        # encoder itself because it needs the output too (MWER training scores its n-best lists on this very pass)
        encode_feature, encode_len = self.encoder(audio_feature, feature_len) if encoded is None else encoded

        if self.enable_ctc:
            # (The head depends on the encoder only, like the decoder loop below, so it was tried on a second stream
            # beside the loop - round 3 at equal priority, round 4 with the loop on a high-priority stream: the loop's
            # kernels lose what the head gains, 109.0 vs 109.1 ms/step; profiles/r04_head_beside_loop_priorities.log.)
            ctc_output = ops.log_softmax(
                ops.linear(encode_feature, self.ctc_layer.weight, self.ctc_layer.bias))

        if self.enable_att:
            # Init (init char = <SOS>, reset all rnn state and cell) - src/asr.py:101-105
            W = self.pre_embed.weight
            last_char = dops.embedding(
                torch.zeros((bs), dtype=torch.long, device=encode_feature.device), W)
            teacher_ids = teacher
            if (teacher is not None) and (0 < tf_rate < 1) and (emb_decoder is None) \
                    and teacher.shape[1] >= decode_step and sops.supported_loop(self.attention, self.decoder) \
                    and not (self.training and (self.decoder.dropout > 0 or self.embed_drop.p > 0)):
                # scheduled sampling through the fused loop, in two passes (see _scheduled_sampling_inputs)
                self.attention.reset_mem()
                key, value = self._speller_memory(encode_feature, encode_len)
                mixed_ids = self._scheduled_sampling_inputs(key.detach(), value.detach(), encode_len, last_char.detach(),
                                                            teacher_ids, decode_step, tf_rate)
                att_output, att_seq, states = self._teacher_forced_loop(
                    encode_feature, encode_len, last_char, self._embed_drop(dops.embedding(mixed_ids, W)),
                    decode_step, memory=(key, value))
                return ctc_output, encode_len, att_output, att_seq, (states if get_dec_state else None)
            if teacher is not None:
                teacher = self._embed_drop(dops.embedding(teacher, W))
            if (teacher is not None) and (tf_rate == 1) and (emb_decoder is None) \
                    and teacher.shape[1] >= decode_step - 1 \
                    and sops.supported_train_loop(self.attention, self.decoder, self.training):
                # the whole teacher-forced loop as one autograd node (csrc/speller.hip)
                self.attention.reset_mem()
                att_output, att_seq, states = self._teacher_forced_loop(
                    encode_feature, encode_len, last_char, teacher, decode_step)
                return ctc_output, encode_len, att_output, att_seq, (states if get_dec_state else None)
            if (teacher is None) and (emb_decoder is None) and (not torch.is_grad_enabled()) \
                    and sops.supported_loop(self.attention, self.decoder):
                # greedy inference (validation / greedy test decoding, src/asr.py:136-142): one fused C
                # call per step for attention + decoder cell
                self.attention.reset_mem()
                att_output, att_seq, states = self._greedy_loop(encode_feature, encode_len, last_char,
                                                                decode_step)
                return ctc_output, encode_len, att_output, att_seq, (states if get_dec_state else None)
            self.decoder.init_state(bs, max_steps=decode_step)
            self.attention.reset_mem()
            att_seq, output_seq, state_seq = [], [], []

            # full teacher forcing: the vocabulary projection of all L steps is ONE GEMM after the
            # loop instead of L small ones (same math; src/asr.py:220 applies it per step)
            defer_char = (teacher is not None) and (tf_rate == 1) and (emb_decoder is None)

            for t in range(decode_step):
                attn, context = self.attention(self.decoder.get_query(), encode_feature, encode_len)
                decoder_input = dops.concat_last(last_char, context)
                cur_char, d_state = self.decoder(decoder_input, project=not defer_char)
                if teacher is not None:
                    if (tf_rate == 1) or (torch.rand(1).item() <= tf_rate):
                        last_char = teacher[:, t, :]
                    else:
                        with torch.no_grad():
                            if (emb_decoder is not None) and emb_decoder.apply_fuse:
                                _, cur_prob = emb_decoder(d_state, cur_char, return_loss=False)
                            else:
                                cur_prob = ops.log_softmax(cur_char).exp()
                            sampled_char = Categorical(cur_prob).sample()
                        last_char = self._embed_drop(dops.embedding(sampled_char, W))
                else:
                    if (emb_decoder is not None) and emb_decoder.apply_fuse:
                        _, cur_char = emb_decoder(d_state, cur_char, return_loss=False)
                    last_char = dops.embedding(ops.argmax(cur_char), W)

                output_seq.append(cur_char)
                state_seq.append(d_state)
                att_seq.append(attn)

            if defer_char:
                states = dops.stack_steps(state_seq)                                  # [B,L,D]
                # Decoder.forward applies final_dropout to the state that feeds char_trans
                # (src/asr.py:220); one mask over [B,L,D] = L independent per-step masks
                states = ops.dropout(states, self.decoder.dropout, self.training)
                att_output = ops.linear(states, self.decoder.char_trans.weight,
                                        self.decoder.char_trans.bias)                 # [B,L,V]
            else:
                att_output = dops.stack_steps(output_seq)                             # [B,L,V]
            N, T = att_seq[0].shape[1], att_seq[0].shape[2]
            att_seq = dops.stack_steps([a.reshape(bs * N, T) for a in att_seq]) \
                .view(bs, N, decode_step, T)                                          # [B,N,L,T]
            if get_dec_state:
                dec_state = dops.stack_steps(state_seq)

        return ctc_output, encode_len, att_output, att_seq, dec_state

    def _speller_memory(self, encode_feature, encode_len):
        ''' key / value projections of the encoder memory (src/asr.py:277-288) + the attention's length mask '''
        att = self.attention
        att.att_layer.compute_mask(encode_feature, encode_len.to(encode_feature.device))
        key = ops.tanh(ops.linear(encode_feature, att.proj_k.weight, att.proj_k.bias))
        value = ops.tanh(ops.linear(encode_feature, att.proj_v.weight, att.proj_v.bias)) \
            if att.v_proj else encode_feature
        return key, value

    def _scheduled_sampling_inputs(self, key, value, encode_len, sos_emb, teacher_ids, decode_step, tf_rate):
        ''' 0 < tf_rate < 1 (src/asr.py:119-135): the token fed to step t + 1 is the teacher's with probability
            tf_rate, else one SAMPLED from the model's own softmax at step t - no gradient flows through the draw, so
            the training step is the teacher-forced step on the MIXED token sequence.  Pass 1 (here, no autograd): the
            loop one fused step at a time (asrk_speller_step_f32), taking the reference's decisions and draws in the
            reference's order (one torch.rand(1) per step, Categorical.sample on the steps that sample); pass 2 (the
            caller): the fused teacher-forced loop on the mixed sequence, forward and backward.  -> ids [B, L] '''
        att, dec = self.attention, self.decoder
        bs, ts, _ = key.shape
        W = self.pre_embed.weight.detach()
        mixed = teacher_ids[:, :decode_step].clone()
        with torch.no_grad():
            st = sops.SpellerStepper(att, dec, key, value, encode_len.to(key.device), bs, shared=False)
            st.h[0].zero_()
            st.c[0].zero_()
            prev_att = att.att_layer.uniform_init(bs, ts, key.device)
            last_char = sos_emb
            for t in range(decode_step):
                attn, _, x, c = st.step(last_char, prev_att)
                if torch.rand(1).item() > tf_rate:
                    cur_char = ops.linear(x, dec.char_trans.weight, dec.char_trans.bias)
                    mixed[:, t] = Categorical(ops.log_softmax(cur_char).exp()).sample()
                last_char = dops.embedding(mixed[:, t].contiguous(), W)
                prev_att = attn.clone()
                st.h[0].copy_(x)
                st.c[0].copy_(c)
        return mixed

    def _teacher_forced_loop(self, encode_feature, encode_len, sos_emb, teacher_emb, decode_step, memory=None):
        ''' src/asr.py:112-148 with tf_rate == 1 -> (att_output [B,L,V], att_seq [B,1,L,T], states [B,L,D]) '''
        att, dec = self.attention, self.decoder
        enc_len = encode_len.to(encode_feature.device)
        key, value = memory if memory is not None else self._speller_memory(encode_feature, encode_len)
        al = att.att_layer
        N = att.num_head
        if N > 1:                               # the heads' rows b * N + n, built as src/asr.py:294-304 builds them
            key = HeadSplitFn.apply(key, N)
            value = HeadSplitFn.apply(value, N) if att.v_proj else RepeatBatchFn.apply(value, N)
        w_ih, w_hh, b_ih, b_hh = dec.layers.layer_params(0)
        if not dec.enable_cell:                 # GRU decoder: the loop's four-rows-per-unit layout (speller_ops)
            w_ih, w_hh, b_ih, b_hh = sops.stack_gru_params(w_ih, w_hh, b_ih, b_hh)
        upper = [p_ for l in range(1, dec.layer) for p_ in dec.layers.layer_params(l)]     # stacked LSTM decoder
        loc_w = (al.loc_conv.weight, al.loc_proj.weight, al.gen_energy.weight, al.gen_energy.bias) \
            if att.mode == 'loc' else (None, None, None, None)                             # None: dot-product energies
        merge = (att.merge_head.weight, att.merge_head.bias) if N > 1 else (None, None)
        states, att_seq = sops.SpellerLoopFn.apply(
            key, value, enc_len, sos_emb, teacher_emb, att.proj_q.weight, att.proj_q.bias, *loc_w,
            w_ih, w_hh, b_ih, b_hh, decode_step, al.temperature, 0 if dec.enable_cell else 1, N, *merge, *upper)
        # module state as the step-by-step loop leaves it (decode-time callers read these)
        att.key, att.value = key, value
        al.prev_att = att_seq.detach()[:, :, -1, :]
        x = ops.dropout(states, dec.dropout, self.training)       # Decoder.final_dropout (src/asr.py:220)
        att_output = ops.linear(x, dec.char_trans.weight, dec.char_trans.bias)
        return att_output, att_seq, states

    @torch.no_grad()
    def score_hypotheses(self, encode_feature, encode_len, row_mem, ids, lens, workspace_mb=1024):
        ''' Attention-decoder log-probabilities of R given token sequences (second-pass rescoring), teacher-forced in
            eval mode - the arithmetic of forward(..., tf_rate=1, teacher=ids).  encode_feature [U,T',D] / encode_len
            [U]: the encoder's output; row r is scored against utterance row_mem[r]; ids [R,L] int64: the hypotheses
            with <eos> appended, zero-padded; lens [R]: their lengths, <eos> included.
            -> (tok_logp f32 [R,L]: log softmax(att_logits_t)[ids[r,t]], 0 on padding; s_att f64 [R]: their sums).
            The attention's key / value projections are built once per utterance and gathered per row; the loop is the
            fused teacher-forced loop where forward() would take it (sops.supported_train_loop), else forward()'s
            step-by-step loop on the gathered encoder rows.  The vocabulary logits exist for one chunk of whole
            hypotheses at a time (repeated memory + logits of a chunk stay below workspace_mb) and are reduced by
            ops.seq_logp.  Rows go through in blocks of SCORE_BLOCK whatever the workspace is, so chunking changes no
            value. '''
        if not self.enable_att:
            raise RuntimeError('ASR.score_hypotheses needs the attention decoder: this model has ctc_weight = 1')
        if self.training:
            raise RuntimeError('ASR.score_hypotheses scores in eval mode: call model.eval() first')
        att, dec, al = self.attention, self.decoder, self.attention.att_layer
        dev = encode_feature.device
        ids = torch.as_tensor(ids).to(device=dev, dtype=torch.int64)
        R, L = ids.shape
        tok_all = torch.zeros((R, L), dtype=torch.float32, device=dev)
        seq_all = torch.zeros((R,), dtype=torch.float64, device=dev)
        if R == 0 or L == 0:
            return tok_all, seq_all
        lens = torch.as_tensor(lens).to(device=dev, dtype=torch.int64)
        row_mem = torch.as_tensor(row_mem).to(device=dev, dtype=torch.int64)
        enc_len = encode_len.to(dev)
        target = torch.where(torch.arange(L, device=dev).unsqueeze(0) < lens.unsqueeze(1), ids,
                             torch.full_like(ids, -1))
        T = encode_feature.shape[1]
        W = self.pre_embed.weight
        fused = sops.supported_train_loop(att, dec, False)
        att.reset_mem()
        if fused:
            key, value = self._speller_memory(encode_feature, encode_len)
            mem_floats = T * (key.shape[2] + value.shape[2])
        else:
            mem_floats = T * (encode_feature.shape[2] + att.num_head * (att.dim + att.v_dim))
        # Every launch sees exactly SCORE_BLOCK rows (the last block is filled up with copies of its first row): GEMM
        # and step kernels pick their variant by the row count, so a launch shape that followed the chunk size would
        # let workspace_mb change low-order bits.  A chunk is a whole number of blocks; it decides only how much
        # repeated memory exists at a time.
        B = SCORE_BLOCK
        Rp = -(-R // B) * B
        if Rp > R:
            fill = (torch.arange(R, Rp, device=dev) // B) * B          # the first row of the block a filler sits in
            row_mem, ids = torch.cat([row_mem, row_mem[fill]]), torch.cat([ids, ids[fill]])
            target = torch.cat([target, target[fill]])
            tok_all = torch.zeros((Rp, L), dtype=torch.float32, device=dev)
            seq_all = torch.zeros((Rp,), dtype=torch.float64, device=dev)
        per_row = 4 * (2 * mem_floats + L * (self.vocab_size + 2 * dec.dim * dec.layer))
        chunk = max(1, int(workspace_mb * 2 ** 20) // (per_row * B)) * B
        sos_emb = dops.embedding(torch.zeros((B,), dtype=torch.long, device=dev), W)
        seg = torch.arange(B + 1, dtype=torch.int64, device=dev) * L
        self.score_chunks = -(-Rp // chunk)       # how many chunks the last call took (tools / tests read it)
        for c0 in range(0, Rp, chunk):
            rows = row_mem[c0:c0 + chunk]
            len_chunk = enc_len.index_select(0, rows)
            if fused:
                key_chunk, value_chunk = key.index_select(0, rows), value.index_select(0, rows)
            else:
                feat_chunk = encode_feature.index_select(0, rows)
            for b0 in range(0, rows.numel(), B):
                r0 = c0 + b0
                len_rows = len_chunk[b0:b0 + B]
                teacher = dops.embedding(ids[r0:r0 + B].contiguous(), W)
                att.reset_mem()
                if fused:
                    key_rows, value_rows = key_chunk[b0:b0 + B], value_chunk[b0:b0 + B]
                    al.compute_mask(key_rows, len_rows)
                    logits, _, _ = self._teacher_forced_loop(key_rows, len_rows, sos_emb, teacher, L,
                                                             memory=(key_rows, value_rows))
                else:
                    feat_rows = feat_chunk[b0:b0 + B]
                    dec.init_state(B)
                    last_char, state_seq = sos_emb, []
                    for t in range(L):
                        _, context = att(dec.get_query(), feat_rows, len_rows)
                        _, d_state = dec(dops.concat_last(last_char, context), project=False)
                        last_char = teacher[:, t, :]
                        state_seq.append(d_state)
                    states = dops.stack_steps(state_seq)                                  # [B,L,D]
                    logits = ops.linear(states, dec.char_trans.weight, dec.char_trans.bias)
                tok, seq = ops.seq_logp(logits.reshape(B * L, self.vocab_size), target[r0:r0 + B].reshape(-1), seg)
                tok_all[r0:r0 + B] = tok.view(B, L)
                seq_all[r0:r0 + B] = seq
        att.reset_mem()
        return tok_all[:R], seq_all[:R]

    def hypothesis_logp(self, encode_feature, encode_len, ids, lens):
        ''' score_hypotheses with a gradient (MWER training, src/mwer.py): the attention decoder's log-probability of
            N hypotheses per utterance, teacher-forced in WHATEVER mode the module is in (training: dropout live).
            encode_feature [U,T',D] / encode_len [U]: the encoder's output (of the training forward); ids [N*U,L] int64:
            the hypotheses with <eos> appended, zero-padded, row n*U + u = hypothesis n of utterance u (the order of
            RepeatBatchFn); lens [N*U]: their lengths, <eos> included.  -> s float64 [N*U], the sums of
            log softmax(att_logits_t)[ids[r,t]] over t < lens[r], added in ascending t.
            The key / value projections are built once per utterance and repeated by RepeatBatchFn (whose backward adds
            the N copies in a fixed order); one loop runs over all N*U rows - the fused teacher-forced loop where
            forward() would take it, else forward()'s step-by-step loop - then one vocabulary projection, reduced by
            ops.SeqLogpFn, whose backward writes the gradient over the logits (nothing else reads them). '''
        if not self.enable_att:
            raise RuntimeError('ASR.hypothesis_logp needs the attention decoder: this model has ctc_weight = 1')
        att, dec = self.attention, self.decoder
        dev = encode_feature.device
        ids = torch.as_tensor(ids).to(device=dev, dtype=torch.int64).contiguous()
        lens = torch.as_tensor(lens).to(device=dev, dtype=torch.int64)
        R, L = ids.shape
        U = encode_feature.shape[0]
        if R == 0 or L == 0 or R % U != 0:
            raise ValueError('ASR.hypothesis_logp: ids must be [N*U, L] with N, L >= 1 (got {} rows for {} '
                             'utterances)'.format(R, U))
        N = R // U
        target = torch.where(torch.arange(L, device=dev).unsqueeze(0) < lens.unsqueeze(1), ids,
                             torch.full_like(ids, -1))
        len_rows = encode_len.to(dev).repeat(N)
        W = self.pre_embed.weight
        sos_emb = dops.embedding(torch.zeros((R,), dtype=torch.long, device=dev), W)
        teacher = self._embed_drop(dops.embedding(ids, W))
        att.reset_mem()
        key, value = self._speller_memory(encode_feature, encode_len)
        key_rows, value_rows = RepeatBatchFn.apply(key, N), RepeatBatchFn.apply(value, N)
        if sops.supported_train_loop(att, dec, self.training):
            att.att_layer.compute_mask(key_rows, len_rows)
            logits, _, _ = self._teacher_forced_loop(key_rows, len_rows, sos_emb, teacher, L,
                                                     memory=(key_rows, value_rows))
        else:
            dec.init_state(R, max_steps=L)
            att.load_memory(key_rows, value_rows, len_rows)
            last_char, state_seq = sos_emb, []
            for t in range(L):
                _, context = att(dec.get_query(), key_rows, len_rows)
                _, d_state = dec(dops.concat_last(last_char, context), project=False)
                last_char = teacher[:, t, :]
                state_seq.append(d_state)
            states = ops.dropout(dops.stack_steps(state_seq), dec.dropout, self.training)     # [R,L,D]
            logits = ops.linear(states, dec.char_trans.weight, dec.char_trans.bias)
        seg = torch.arange(R + 1, dtype=torch.int64, device=dev) * L
        s = ops.SeqLogpFn.apply(logits.reshape(R * L, self.vocab_size), target.reshape(-1), seg, True)
        att.reset_mem()
        return s

    def _greedy_loop(self, encode_feature, encode_len, sos_emb, decode_step):
        ''' argmax-feedback decoding without autograd -> (att_output [B,L,V], att_seq [B,1,L,T], states) '''
        att, dec = self.attention, self.decoder
        bs, ts, _ = encode_feature.shape
        dev = encode_feature.device
        enc_len = encode_len.to(dev)
        att.att_layer.compute_mask(encode_feature, enc_len)
        key = ops.tanh(ops.linear(encode_feature, att.proj_k.weight, att.proj_k.bias))
        value = ops.tanh(ops.linear(encode_feature, att.proj_v.weight, att.proj_v.bias)) \
            if att.v_proj else encode_feature
        st = sops.SpellerStepper(att, dec, key, value, enc_len, bs, shared=False)
        st.h[0].zero_()
        st.c[0].zero_()
        prev_att = att.att_layer.uniform_init(bs, ts, dev)
        W = self.pre_embed.weight
        f = dict(dtype=torch.float32, device=dev)
        att_output = torch.empty((bs, decode_step, self.vocab_size), **f)
        att_seq = torch.empty((bs, 1, decode_step, ts), **f)
        states = torch.empty((bs, decode_step, dec.dim), **f)
        last_char = sos_emb
        for t in range(decode_step):
            attn, _, x, c = st.step(last_char, prev_att)
            cur_char = ops.linear(ops.dropout(x, dec.dropout, self.training), dec.char_trans.weight,
                                  dec.char_trans.bias)
            last_char = dops.embedding(ops.argmax(cur_char), W)
            att_output[:, t].copy_(cur_char)
            att_seq[:, :, t].copy_(attn)
            states[:, t].copy_(x)
            prev_att = att_seq[:, :, t].contiguous()
            st.h[0].copy_(x)
            st.c[0].copy_(c)
        att.key, att.value = key, value
        att.att_layer.prev_att = prev_att
        dec.hidden_state = (st.h[0].clone().unsqueeze(0), st.c[0].clone().unsqueeze(0)) if dec.enable_cell \
            else st.h[0].clone().unsqueeze(0)
        return att_output, att_seq, states

    def _embed_drop(self, x):
        return ops.dropout(x, self.embed_drop.p, self.training)


class Decoder(nn.Module):
    ''' Decoder (a.k.a. Speller in LAS) (reference: src/asr.py:158-221) '''

    def __init__(self, input_dim, vocab_size, module, dim, layer, dropout):
        super(Decoder, self).__init__()
        self.in_dim = input_dim
        self.layer = layer
        self.dim = dim
        self.dropout = dropout

        assert module in ['LSTM', 'GRU'], NotImplementedError
        self.hidden_state = None
        self.enable_cell = module == 'LSTM'

        # parameters named exactly like nn.LSTM(input_dim, dim, num_layers=layer) (decode.py reads
        # decoder.layers.bias_ih_l{l}); the math is dops.LSTMCellStepFn
        self.layers = RNNParams(module, input_dim, dim, num_layers=layer, dropout=dropout,
                                batch_first=True)
        self.char_trans = nn.Linear(dim, vocab_size)
        self.final_dropout = nn.Dropout(dropout)
        self._tapes = None

    def init_state(self, bs, max_steps=None):
        ''' Set all hidden states to zeros '''
        device = next(self.parameters()).device
        z = lambda: torch.zeros((self.layer, bs, self.dim), device=device)
        self.hidden_state = (z(), z()) if self.enable_cell else z()
        self._tapes = None
        if self.enable_cell and max_steps is not None and torch.is_grad_enabled():
            self._tapes = []
            for l in range(self.layer):
                w = self.layers.layer_params(l)
                tape = dops.CellTape(*[ops._f32c(p) for p in w], bs, max_steps)
                token = dops.CellHubFn.apply(tape, *w)
                self._tapes.append((tape, token))
        return self.get_state()

    def set_state(self, hidden_state):
        ''' Set all hidden states/cells, for decoding purpose'''
        device = next(self.parameters()).device
        if self.enable_cell:
            self.hidden_state = (hidden_state[0].to(device), hidden_state[1].to(device))
        else:
            self.hidden_state = hidden_state.to(device)

    def get_state(self):
        ''' Return all hidden states/cells, for decoding purpose'''
        if self.enable_cell:
            return (self.hidden_state[0].cpu(), self.hidden_state[1].cpu())
        else:
            return self.hidden_state.cpu()

    def get_query(self):
        ''' Return state of all layers as query for attention '''
        h = self.hidden_state[0] if self.enable_cell else self.hidden_state
        if self.layer == 1:
            return h[0]
        return h.transpose(0, 1).reshape(-1, self.dim * self.layer)

    def forward(self, x, project=True):
        ''' One decode step through the stacked cells, then transform into vocab '''
        if not self.enable_cell:
            return self._forward_gru(x, project)
        hs, cs = [], []
        h_all, c_all = self.hidden_state
        bs = x.shape[0]
        for l in range(self.layer):
            if self._tapes is not None and self._tapes[l][0].used < self._tapes[l][0].cap:
                tape, token = self._tapes[l]
            else:  # stepping outside ASR.forward (beam search) or beyond the planned length
                w = self.layers.layer_params(l)
                tape = dops.CellTape(*[ops._f32c(p) for p in w], bs, 1)
                token = dops.CellHubFn.apply(tape, *w)
            h, c = dops.LSTMCellStepFn.apply(tape, token, x, h_all[l], c_all[l])
            hs.append(h)
            cs.append(c)
            x = h
            if l + 1 < self.layer:
                x = ops.dropout(x, self.dropout, self.training)   # nn.LSTM inter-layer dropout
        if self.layer == 1:
            self.hidden_state = (hs[0].unsqueeze(0), cs[0].unsqueeze(0))
        else:
            self.hidden_state = (torch.stack(hs, 0), torch.stack(cs, 0))
        char = None
        if project:
            char = ops.linear(ops.dropout(x, self.dropout, self.training), self.char_trans.weight,
                              self.char_trans.bias)
        return char, x

    def _forward_gru(self, x, project):
        ''' stacked nn.GRU cells, one step (state = h only) '''
        from .. import gru_ops
        hs = []
        for l in range(self.layer):
            h = gru_ops.gru_cell(x, self.hidden_state[l], *self.layers.layer_params(l))
            hs.append(h)
            x = h
            if l + 1 < self.layer:
                x = ops.dropout(x, self.dropout, self.training)
        self.hidden_state = hs[0].unsqueeze(0) if self.layer == 1 else torch.stack(hs, 0)
        char = None
        if project:
            char = ops.linear(ops.dropout(x, self.dropout, self.training), self.char_trans.weight,
                              self.char_trans.bias)
        return char, x


class Attention(nn.Module):
    ''' Attention mechanism (reference: src/asr.py:224-313).
        Input : decoder state [B, q_dim], encoder memory [B, T, v_dim], lengths [B]
        Output: attention score [B, num_head, T], context vector [B, v_dim] '''

    def __init__(self, v_dim, q_dim, mode, dim, num_head, temperature, v_proj,
                 loc_kernel_size, loc_kernel_num):
        super(Attention, self).__init__()
        self.v_dim = v_dim
        self.dim = dim
        self.mode = mode.lower()
        self.num_head = num_head

        self.proj_q = nn.Linear(q_dim, dim * num_head)
        self.proj_k = nn.Linear(v_dim, dim * num_head)
        self.v_proj = v_proj
        if v_proj:
            self.proj_v = nn.Linear(v_dim, v_dim * num_head)

        if self.mode == 'dot':
            self.att_layer = ScaleDotAttention(temperature, self.num_head)
        elif self.mode == 'loc':
            self.att_layer = LocationAwareAttention(
                loc_kernel_size, loc_kernel_num, dim, num_head, temperature)
        else:
            raise NotImplementedError

        if self.num_head > 1:
            self.merge_head = nn.Linear(v_dim * num_head, v_dim)

        self.key = None
        self.value = None
        self.mask = None
        self._tape = None
        self._token = None

    def reset_mem(self):
        self.key = None
        self.value = None
        self.mask = None
        self._tape = None
        self._token = None
        self.att_layer.reset_mem()

    def set_mem(self, prev_attn):
        self.att_layer.set_mem(prev_attn)

    def _split_heads(self, x, bs, ts, d):
        ''' [B,T,N*d] -> [B*N,T,d] (src/asr.py:294-301) '''
        N = self.num_head
        out = torch.empty((bs * N, ts, d), dtype=torch.float32, device=x.device)
        xc = ops._f32c(x)
        for b in range(bs):  # out[b*N+n, t, :] = x[b, t, n*d:(n+1)*d]
            ops.copy3d(xc[b], out[b * N:], N, ts, d, d, N * d, ts * d, d)
        return out

    def build_memory(self, enc_feat, enc_len):
        ''' key/value cache + padded-frame mask of src/asr.py:285-304 -> (AttnTape, key, value, loc_w) '''
        enc_len = enc_len.to(enc_feat.device)
        self.att_layer.compute_mask(enc_feat, enc_len)
        key = ops.tanh(ops.linear(enc_feat, self.proj_k.weight, self.proj_k.bias))
        value = ops.tanh(ops.linear(enc_feat, self.proj_v.weight, self.proj_v.bias)) \
            if self.v_proj else enc_feat
        return self._memory_tape(key, value, enc_len)

    def _memory_tape(self, key, value, enc_len):
        ''' the tape of the step-by-step loop from projected key / value rows [B,T,N*d] (the mask is already set) '''
        N = self.num_head
        if N > 1:
            key = HeadSplitFn.apply(key, N)
            if self.v_proj:
                value = HeadSplitFn.apply(value, N)
            else:
                value = RepeatBatchFn.apply(value, N)   # reference: value.repeat(N,1,1)
        loc_w = ()
        if self.mode == 'loc':
            al = self.att_layer
            loc_w = (al.loc_conv.weight, al.loc_proj.weight, al.gen_energy.weight.view(-1),
                     al.gen_energy.bias)
        tape = dops.AttnTape(self.mode, ops._f32c(key), ops._f32c(value), enc_len, N,
                             self.att_layer.temperature,
                             tuple(ops._f32c(w) for w in loc_w) if loc_w else None)
        return tape, key, value, loc_w

    def load_memory(self, key, value, enc_len):
        ''' what the first forward() call of a sequence does, from key / value projections the caller already holds
            (ASR.hypothesis_logp: projected once per utterance, then repeated per hypothesis): forward() then steps
            over these rows and never projects the encoder output itself '''
        enc_len = enc_len.to(key.device)
        self.att_layer.compute_mask(key, enc_len)
        self._tape, key, value, loc_w = self._memory_tape(key, value, enc_len)
        self.key, self.value = key, value
        self._token = dops.AttnHubFn.apply(self._tape, key, value, *loc_w)

    def forward(self, dec_state, enc_feat, enc_len):
        bs, ts, _ = enc_feat.shape
        N = self.num_head
        query = ops.tanh(ops.linear(dec_state, self.proj_q.weight, self.proj_q.bias))
        query = query.view(bs * N, self.dim)  # BNxD

        if self.key is None:
            self._tape, key, value, loc_w = self.build_memory(enc_feat, enc_len)
            self.key, self.value = key, value
            self._token = dops.AttnHubFn.apply(self._tape, key, value, *loc_w)

        prev_att = None
        if self.mode == 'loc':
            if self.att_layer.prev_att is None:
                self.att_layer.prev_att = self.att_layer.uniform_init(bs, ts, enc_feat.device)
            prev_att = self.att_layer.prev_att
        attn, context = dops.AttnStepFn.apply(self._tape, self._token, query, prev_att)
        if self.mode == 'loc':
            self.att_layer.prev_att = attn
        if N > 1:
            context = context.view(bs, N * self.v_dim)
            context = ops.linear(context, self.merge_head.weight, self.merge_head.bias)
        return attn, context


class HeadSplitFn(torch.autograd.Function):
    ''' [B,T,N*d] -> [B*N,T,d]: view(B,T,N,d).permute(0,2,1,3) of src/asr.py:294-301 '''

    @staticmethod
    def forward(ctx, x, N):
        xc = ops._f32c(x)
        B, T, ND = xc.shape
        d = ND // N
        out = torch.empty((B * N, T, d), dtype=torch.float32, device=x.device)
        for b in range(B):
            ops.copy3d(xc[b], out[b * N:], N, T, d, d, ND, T * d, d)
        ctx.dims = (B, T, N, d)
        return out

    @staticmethod
    def backward(ctx, g):
        B, T, N, d = ctx.dims
        gc = ops._f32c(g)
        out = torch.empty((B, T, N * d), dtype=torch.float32, device=g.device)
        for b in range(B):
            ops.copy3d(gc[b * N:], out[b], N, T, d, T * d, d, d, N * d)
        return out, None


class RepeatBatchFn(torch.autograd.Function):
    ''' x.repeat(N,1,1) for [B,T,D] (src/asr.py:304; rows ordered (n, b) exactly like the reference) '''

    @staticmethod
    def forward(ctx, x, N):
        xc = ops._f32c(x)
        B, T, D = xc.shape
        out = torch.empty((N * B, T, D), dtype=torch.float32, device=x.device)
        for n in range(N):
            ops.copy3d(xc, out[n * B:], 1, B * T, D, 0, D, 0, D)
        ctx.dims = (B, T, D, N)
        return out

    @staticmethod
    def backward(ctx, g):
        B, T, D, N = ctx.dims
        gc = ops._f32c(g)
        out = torch.zeros((B, T, D), dtype=torch.float32, device=g.device)
        for n in range(N):
            ops.copy3d(gc[n * B:], out, 1, B * T, D, 0, D, 0, D, accumulate=True)
        return out, None


class Encoder(nn.Module):
    ''' Encoder (a.k.a. Listener in LAS) (reference: src/asr.py:316-366).  Layers are chained in a
    time-major layout internally ([T,B,D], what the persistent recurrence kernels want); the
    module's own interface stays batch-major like the reference. '''

    def __init__(self, input_size, prenet, module, bidirection, dim, dropout, layer_norm, proj,
                 sample_rate, sample_style):
        super(Encoder, self).__init__()

        self.vgg = prenet == 'vgg'
        self.cnn = prenet == 'cnn'
        self.sample_rate = 1
        assert len(sample_rate) == len(dropout), 'Number of layer mismatch'
        assert len(dropout) == len(dim), 'Number of layer mismatch'
        num_layers = len(dim)
        assert num_layers >= 1, 'Encoder should have at least 1 layer'

        module_list = []
        input_dim = input_size

        if self.vgg:
            vgg_extractor = VGGExtractor(input_size)
            module_list.append(vgg_extractor)
            input_dim = vgg_extractor.out_dim
            self.sample_rate = self.sample_rate * 4
        if self.cnn:
            cnn_extractor = CNNExtractor(input_size, out_dim=dim[0])
            module_list.append(cnn_extractor)
            input_dim = cnn_extractor.out_dim
            self.sample_rate = self.sample_rate * 4

        if module in ['LSTM', 'GRU']:
            for l in range(num_layers):
                module_list.append(RNNLayer(input_dim, module, dim[l], bidirection, dropout[l],
                                            layer_norm[l], sample_rate[l], sample_style, proj[l]))
                input_dim = module_list[-1].out_dim
                self.sample_rate = self.sample_rate * sample_rate[l]
        else:
            raise NotImplementedError

        self.in_dim = input_size
        self.out_dim = input_dim
        self.layers = nn.ModuleList(module_list)

    def supports_packed(self):
        ''' forward(packed=True) is available: every recurrent layer is an LSTM with a hidden size the packed kernel
            takes (GRU layers: no length-aware recurrence yet).  A VGG / CNN prenet does not stand in the way: its
            packed form gives every convolution a per-utterance valid height (forward_bm2tm(packed=True)) '''
        return all(l.supports_packed() for l in self.layers if isinstance(l, RNNLayer))

    def forward(self, input_x, enc_len, packed=False):
        ''' packed=True (inference): input_x [U,T,D] zero-padded, enc_len [U]; every utterance is encoded exactly as
            if it had been passed alone and unpadded (the prenet's forward_bm2tm(packed=True), then
            RNNLayer.forward_tm(packed=True)); a prenet never reads input frames beyond enc_len; output frames beyond an
            utterance's length are zero (LayerNorm / projection outputs there are NOT - consumers mask by length) '''
        if packed:
            if not self.supports_packed():
                raise RuntimeError('Encoder: packed encoding is not available for this configuration')
            layers = list(self.layers)
            if self.vgg or self.cnn:
                # a batch-1 prenet run emits exactly the frames it reports (L // 4): frames == enc_len behind it
                x, enc_len = layers[0].forward_bm2tm(input_x, enc_len, packed=True)
                layers = layers[1:]
            else:
                x = ops.swap_bt(input_x)
            frames = enc_len
            for layer in layers:
                x, enc_len, frames = layer.forward_tm(x, enc_len, packed=True, frames=frames)
            # frames an utterance's own (batch-1) encoder output would have: what everything that walks the output
            # TENSOR of such a run sees (CTC prefix scorer, CTC beam search); == enc_len unless a 'drop' reduction
            # met an odd length
            self.packed_frames = frames
            # inference: nobody polls the recurrence kernels' error word every N steps as the training loop does, and an
            # aborted launch leaves its pooled exchange buffer dirty - ask right here, before anything decodes from x
            ops.check_errors()
            return ops.swap_bt(x), enc_len
        layers = list(self.layers)
        if self.vgg or self.cnn:
            # the prenet reads the batch-major features in place and emits time-major frames
            x, enc_len = layers[0].forward_bm2tm(input_x, enc_len)
            layers = layers[1:]
        else:
            x = ops.swap_bt(input_x)  # [B,T,D] -> [T,B,D] once
        for i, layer in enumerate(layers):
            # a wide LSTM layer whose output goes straight into the next LSTM layer's input projection (no LayerNorm /
            # dropout / projection in between) may write that output as a split panel itself (ops.set_panel_hint)
            nxt = layers[i + 1] if i + 1 < len(layers) else None
            ops.set_panel_hint(isinstance(layer, RNNLayer) and isinstance(nxt, RNNLayer) and layer.rnn_type == 'LSTM'
                               and nxt.rnn_type == 'LSTM' and nxt.bidirection and nxt.layer.hidden_size >= 768
                               and not layer.layer_norm and not layer.proj
                               and not (layer.dropout > 0 and self.training)
                               and (layer.sample_rate == 1 or layer.sample_style == 'concat'))
            x, enc_len = layer.forward_tm(x, enc_len)
        ops.set_panel_hint(False)
        if not torch.is_grad_enabled():
            ops.check_errors()          # decoding / validation: see the packed branch
        return ops.swap_bt(x), enc_len
