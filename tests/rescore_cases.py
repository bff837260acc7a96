"""Inputs shared by the CPU and the GPU rescoring tests: the golden models, three utterances of mixed lengths per model
and the decode settings.  The feature seeds are chosen so that, on the float64 reference alone, adjacent final scores
of every utterance's n-best list lie more than MIN_GAP apart (asserted in tests/test_rescore_cpu.py): the order is then
decided by far more than the f32 tolerance of the GPU path (about 1e-5 on these shapes)."""
import numpy as np
import torch

E2E_CASES = ["las_hybrid_loc", "las_gru", "las_loc_mh"]   # fused LSTM loop / step-by-step GRU / multi-head loc
BEAM, CAND, CTC_W = 6, 8, 0.3
LENS = [37, 26, 15]                                        # feature frames (<= 60), all different
SEEDS = {"las_hybrid_loc": 3, "las_gru": 0, "las_loc_mh": 0}
MIN_GAP = 8e-3


def utterances(case, D, seed=None):
    """-> (feat [3, 37, D] zero-padded float32, feat_len [3] int64)"""
    rs = np.random.RandomState(1000 + SEEDS[case] if seed is None else seed)
    feat = np.zeros((len(LENS), max(LENS), D), dtype=np.float32)
    for u, n in enumerate(LENS):
        feat[u, :n] = rs.randn(n, D).astype(np.float32)
    return torch.from_numpy(feat), torch.tensor(LENS, dtype=torch.int64)


def vocab_range(V):
    return [1] + list(range(3, V))


# the LM tests (las_hybrid_loc, lm_weight 0.3, RNN-LM and n-gram, first pass with and without the LM): with this seed
# adjacent reference scores of all twelve lists are more than 3e-3 apart
LM_SEED = 2025
