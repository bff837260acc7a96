"""Worker of tests/test_rowops_variants_gpu.py (a subprocess, so that ASRK_DETERMINISTIC is read by a fresh library).

    rowops_variants_worker.py <out.npz>   rowops_reference.COLSUM_DET_ROWS through asrk_colsum_f32 with accumulate 0 and 1
                                          (cs_<acc>_<row>, and the plan's cs_variant_<row>, cs_chunks_<row>), and the
                                          LayerNorm parameter gradient of LN_DET_ROWS twice (ln_dw_<row>, ln_db_<row> of the
                                          first run, ln_same_<row> = the second run gave the same bits, ln_chunks_<row>)
"""
import ctypes
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "end-to-end-asr-pytorch_amd"
import rowops_reference as R          # noqa: E402


def main():
    assert os.environ.get("ASRK_DETERMINISTIC") == "1"
    ops = importlib.import_module(PKG + ".ops")
    lib = importlib.import_module(PKG + "._lib")
    L, st, p = ops._L(), ops._stream, ops._p
    out = {}
    for name in R.COLSUM_DET_ROWS:
        c = R.COLSUM_BY_NAME[name]
        buf, out0 = R.colsum_inputs(name)
        xd = torch.from_numpy(buf).cuda()
        xp = xd.data_ptr() + 4 * c.off
        for acc in (0, 1):
            o = torch.from_numpy(out0).cuda() if acc else torch.full((c.N,), float('nan'), device='cuda')
            plan = R.plan(L, R.OP_COLSUM, [xp, o.data_ptr()], [c.M, c.N, c.ldx, acc])
            assert plan['chunks'] == 1 and (plan['gy'] if c.variant != R.NARROW else plan['gx']) == 1, (name, plan)
            lib.check(L.asrk_colsum_f32(ctypes.c_void_p(xp), c.M, c.N, c.ldx, p(o), acc, st()), "colsum")
            ops.check_errors()
            out['cs_%d_%s' % (acc, name)] = o.cpu().numpy()
        out['cs_variant_' + name], out['cs_chunks_' + name] = np.asarray(plan['variant']), np.asarray(plan['chunks'])
    for name in R.LN_DET_ROWS:
        c = R.LN_BY_NAME[name]
        x, w, b, dy = (t.cuda() for t in R.ln_inputs(name))
        plan = R.plan(L, R.OP_LN_PARAM, [], [c.rows, c.D])
        assert plan['chunks'] == 1 and plan['gy'] == 1 and plan['per'] >= c.rows, (name, plan)
        y, mean, rstd = torch.empty_like(x), torch.empty(c.rows, device='cuda'), torch.empty(c.rows, device='cuda')
        lib.check(L.asrk_layer_norm_fwd_f32(p(x), p(w), p(b), p(y), p(mean), p(rstd), c.rows, c.D, c.eps, st()), "ln_fwd")
        runs = []
        for _ in range(2):
            dw = torch.full((c.D,), float('nan'), device='cuda')
            db = torch.full((c.D,), float('nan'), device='cuda')
            lib.check(L.asrk_layer_norm_bwd_f32(p(x), p(w), p(dy), p(mean), p(rstd), None, p(dw), p(db), c.rows, c.D, st()),
                      "ln_bwd")
            ops.check_errors()
            runs.append((dw.cpu().numpy(), db.cpu().numpy()))
        out['ln_dw_' + name], out['ln_db_' + name] = runs[0]
        out['ln_same_' + name] = np.asarray(runs[0][0].tobytes() == runs[1][0].tobytes()
                                            and runs[0][1].tobytes() == runs[1][1].tobytes())
        out['ln_chunks_' + name] = np.asarray(plan['chunks'])
    np.savez(sys.argv[1], **out)
    print('DONE', flush=True)


if __name__ == '__main__':
    main()
