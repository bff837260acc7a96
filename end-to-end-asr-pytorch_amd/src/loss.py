"""Loss options of the training solvers: the top-level `loss:` block of a config.

    loss:
      label_smoothing: 0.1        # attention / LM cross entropy (uniform smoothing), a number in [0, 1)
      ctc_zero_infinity: true     # ASR only: an utterance whose transcript does not fit its encoder frames
                                  # contributes loss 0 and a zero gradient instead of +inf and NaN

An absent block is the defaults (0.0, false): the losses are then built exactly as before."""


class LossOptions:
    KEYS = ('label_smoothing', 'ctc_zero_infinity')

    def __init__(self, label_smoothing=0.0, ctc_zero_infinity=False):
        if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float)) or \
                not 0.0 <= label_smoothing < 1.0:
            raise ValueError('loss: label_smoothing must be a number in [0, 1), got %r' % (label_smoothing,))
        if not isinstance(ctc_zero_infinity, bool):
            raise ValueError('loss: ctc_zero_infinity must be true or false, got %r' % (ctc_zero_infinity,))
        self.label_smoothing = float(label_smoothing)
        self.ctc_zero_infinity = ctc_zero_infinity

    @classmethod
    def from_config(cls, cfg, ctc=True):
        """cfg: the whole yaml config (a mapping).  ctc=False (the LM solver, which has no CTC branch): the block may
        only hold `label_smoothing`."""
        block = cfg.get('loss') if cfg is not None else None
        if block is None:
            return cls()
        if not isinstance(block, dict):
            raise ValueError('loss: expected a mapping, got %r' % (block,))
        keys = cls.KEYS if ctc else cls.KEYS[:1]
        unknown = sorted(set(block) - set(keys), key=str)
        if unknown:
            raise ValueError('loss: unknown key(s) %s (known: %s)' % (unknown, ', '.join(keys)))
        return cls(**block)

    @property
    def active(self):
        return self.label_smoothing > 0.0 or self.ctc_zero_infinity

    def create_msg(self):
        return 'Loss options | label smoothing {:g} | CTC zero_infinity {}'.format(
            self.label_smoothing, 'on' if self.ctc_zero_infinity else 'off')
