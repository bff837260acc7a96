"""Float64 reference of the persistent LSTM / GRU recurrence ALONE, at the level of the C ABI of include/asrk.h
(asrk_lstm_rec_{fwd,bwd}_pyr_f32, asrk_lstm_rec_fwd_len_f32, asrk_gru_rec_{fwd,bwd}_f32): pre-activations in, outputs,
cell states and activated gates out; BPTT written out by hand from dY (in the time-reduced layout) to dG and db.  Plain
torch on the CPU, no GEMM of the layer around it.  tests/test_recurrence_reference_cpu.py pins it to the oracle
(oracle/asr_oracle.py lstm_layer / gru_layer under float64 autograd).

Also the ONE case table of the recurrence variant tests: a row per kernel variant and per edge, each naming the variant
`asrk_lstm_plan_info` must report for it on a 256-CU device (tests/test_recurrence_plan_cpu.py holds the table to
that; tests/test_recurrence_variants_gpu.py runs it).  If a re-tune moves a row to another variant, move the SHAPE."""
import functools
import zlib
from collections import namedtuple

import torch

T = 7            # odd; > 2 steps (parity double buffer, in-kernel re-arm of region s - 2); 7 % 2 and 7 % 3 leave frames
NCU = 256        # the device the table is written for (MI355X)
F32_MFMA, REARM = 1, 2           # ASRK_REC_F32_MFMA, ASRK_REC_REARM
MODES = ((0, 1), (1, 2), (2, 2), (1, 3))     # (pyr_mode, rate): plain, concat r=2, drop r=2, concat r=3
MODE_NAMES = {(0, 1): "plain", (1, 2): "concat2", (2, 2): "drop2", (1, 3): "concat3"}


# ------------------------------------------------------------------------------------------------ time reduction
def reduce_time(Y, mode, r, lens=None):
    """Y [T, B, D] -> Y2 of include/asrk.h: 'concat' [T/r, B, r*D] (trailing frames dropped; with lens every row trims
    lens[b] % r frames by itself, the rest stays zero), 'drop' [ceil(T/r), B, D] = Y[0::r]"""
    Tn, B, D = Y.shape
    if mode == 0:
        return None
    if mode == 2:
        return Y[0::r].clone()
    Y2 = Y.new_zeros(Tn // r, B, r * D)
    for b in range(B):
        n = (Tn if lens is None else int(lens[b])) // r
        Y2[:n, b] = Y[:n * r, b].reshape(n, r * D)
    return Y2


def expand_dy(dY2, mode, r, Tn):
    """gradient w.r.t. Y2 (reduced layout) -> gradient w.r.t. Y [T, B, D]; dropped frames get zero"""
    if mode == 0:
        return dY2.clone()
    if mode == 2:
        dY = dY2.new_zeros(Tn, dY2.shape[1], dY2.shape[2])
        dY[0::r] = dY2
        return dY
    n, B, rD = dY2.shape
    dY = dY2.new_zeros(Tn, B, rD // r)
    dY[:n * r] = dY2.reshape(n, B, r, rD // r).permute(0, 2, 1, 3).reshape(n * r, B, rD // r)
    return dY


def dy_shape(mode, r, Tn, B, D):
    return {0: (Tn, B, D), 1: (Tn // r, B, r * D), 2: (-(-Tn // r), B, D)}[mode]


def _order(Tn, d):
    return range(Tn) if d == 0 else range(Tn - 1, -1, -1)


# ------------------------------------------------------------------------------------------------ LSTM
def lstm_fwd(G, whh, Tn, B, H, ndir):
    """G [T*B, ndir*4H] pre-activations (column = dir*4H + gate*H + unit, gates i,f,g,o), whh: ndir x [4H, H].
    -> Y, C [T, B, ndir*H], gates [T, B, ndir*4H] (activated).  Computes in G's dtype."""
    G = G.reshape(Tn, B, ndir, 4, H)
    Y = G.new_zeros(Tn, B, ndir, H)
    C = G.new_zeros(Tn, B, ndir, H)
    A = torch.zeros_like(G)
    for d in range(ndir):
        w = whh[d].to(G.dtype)
        h, c = G.new_zeros(B, H), G.new_zeros(B, H)
        for t in _order(Tn, d):
            g = G[t, :, d] + (h @ w.t()).reshape(B, 4, H)
            i, f, o = torch.sigmoid(g[:, 0]), torch.sigmoid(g[:, 1]), torch.sigmoid(g[:, 3])
            gg = torch.tanh(g[:, 2])
            c = f * c + i * gg
            h = o * torch.tanh(c)
            A[t, :, d] = torch.stack([i, f, gg, o], 1)
            Y[t, :, d], C[t, :, d] = h, c
    return Y.reshape(Tn, B, ndir * H), C.reshape(Tn, B, ndir * H), A.reshape(Tn, B, ndir * 4 * H)


def lstm_fwd_len(G, whh, lens, Tn, B, H, ndir):
    """the `lens` form: every row alone and unpadded (the reverse direction starts at its own last frame); frames
    t >= lens[b] stay zero here (the kernel does not write them) -> Y, C, gates, valid [T, B] mask"""
    G = G.reshape(Tn, B, ndir * 4 * H)
    Y, C = G.new_zeros(Tn, B, ndir * H), G.new_zeros(Tn, B, ndir * H)
    A = torch.zeros_like(G)
    valid = torch.zeros(Tn, B, dtype=torch.bool)
    for b in range(B):
        n = int(lens[b])
        y, c, a = lstm_fwd(G[:n, b:b + 1].reshape(n, -1), whh, n, 1, H, ndir)
        Y[:n, b], C[:n, b], A[:n, b], valid[:n, b] = y[:, 0], c[:, 0], a[:, 0], True
    return Y, C, A, valid


def lstm_bwd(gates, whh, C, dY, Tn, B, H, ndir):
    """BPTT: activated gates, cell states, dY [T, B, ndir*H] (already expanded) -> dG [T, B, ndir*4H], db [ndir*4H]"""
    A = gates.reshape(Tn, B, ndir, 4, H)
    C = C.reshape(Tn, B, ndir, H)
    dY = dY.reshape(Tn, B, ndir, H)
    dG = torch.zeros_like(A)
    for d in range(ndir):
        w = whh[d].to(A.dtype)
        order = list(_order(Tn, d))
        dh_next, dc_next = A.new_zeros(B, H), A.new_zeros(B, H)
        for k in range(Tn - 1, -1, -1):
            t = order[k]
            i, f, g, o = A[t, :, d, 0], A[t, :, d, 1], A[t, :, d, 2], A[t, :, d, 3]
            c_prev = C[order[k - 1], :, d] if k > 0 else torch.zeros_like(i)
            tc = torch.tanh(C[t, :, d])
            dh = dY[t, :, d] + dh_next
            dc = dc_next + dh * o * (1 - tc * tc)
            dg4 = torch.stack([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g),
                               dh * tc * o * (1 - o)], 1)
            dG[t, :, d] = dg4
            dc_next = dc * f
            dh_next = dg4.reshape(B, 4 * H) @ w
    dG = dG.reshape(Tn, B, ndir * 4 * H)
    return dG, dG.sum((0, 1))


# ------------------------------------------------------------------------------------------------ GRU
def gru_fwd(G, whh, Tn, B, H, ndir):
    """G per direction: a_r | a_z | a_n | b_hn (every row); whh: ndir x [3H, H] -> Y [T, B, ndir*H],
    gates [T, B, ndir*4H] = r | z | n | W_hn h_{t-1} + b_hn"""
    G = G.reshape(Tn, B, ndir, 4, H)
    Y = G.new_zeros(Tn, B, ndir, H)
    A = torch.zeros_like(G)
    for d in range(ndir):
        w = whh[d].to(G.dtype)
        h = G.new_zeros(B, H)
        for t in _order(Tn, d):
            gh = (h @ w.t()).reshape(B, 3, H)
            r, z = torch.sigmoid(G[t, :, d, 0] + gh[:, 0]), torch.sigmoid(G[t, :, d, 1] + gh[:, 1])
            q = gh[:, 2] + G[t, :, d, 3]
            n = torch.tanh(G[t, :, d, 2] + r * q)
            h = (1 - z) * n + z * h
            A[t, :, d] = torch.stack([r, z, n, q], 1)
            Y[t, :, d] = h
    return Y.reshape(Tn, B, ndir * H), A.reshape(Tn, B, ndir * 4 * H)


def gru_bwd(gates, whh, Y, dY, Tn, B, H, ndir):
    """-> dG [T, B, ndir*4H] = dr | dz | dn | dn*r (pre-activation gradients), db [ndir*4H] their column sums"""
    A = gates.reshape(Tn, B, ndir, 4, H)
    Y = Y.reshape(Tn, B, ndir, H)
    dY = dY.reshape(Tn, B, ndir, H)
    dG = torch.zeros_like(A)
    for d in range(ndir):
        w = whh[d].to(A.dtype)
        order = list(_order(Tn, d))
        dh_next = A.new_zeros(B, H)
        for k in range(Tn - 1, -1, -1):
            t = order[k]
            r, z, n, q = A[t, :, d, 0], A[t, :, d, 1], A[t, :, d, 2], A[t, :, d, 3]
            h_prev = Y[order[k - 1], :, d] if k > 0 else torch.zeros_like(r)
            dh = dY[t, :, d] + dh_next
            dn = dh * (1 - z) * (1 - n * n)
            dr = dn * q * r * (1 - r)
            dz = dh * (h_prev - n) * z * (1 - z)
            dG[t, :, d] = torch.stack([dr, dz, dn, dn * r], 1)
            dh_next = dh * z + torch.cat([dr, dz, dn * r], 1) @ w
    dG = dG.reshape(Tn, B, ndir * 4 * H)
    return dG, dG.sum((0, 1))


# ------------------------------------------------------------------------------------------------ the case table
# variant: forward ('f32' | 'bf', MT, NT, KGW, db); backward ('f32' | 'bf', UB, NT, RK), as asrk_lstm_plan_info reports
# them: for the bf16x6 forward kernel KGW is the template's KSW = H / 128, for the bf16x6 backward kernel RK is 0.  launches: what plan_info must report (1 unless the row is about the
# several-launches fallback).  gru: run the row through the GRU entry points too.  lens: run the `lens` form too.
Row = namedtuple("Row", "name bwd B H ndir flags variant launches mode gru lens knobs")


def _rows():
    rows = []

    def add(name, bwd, B, H, ndir, variant, flags=0, launches=1, gru=False, lens=False, knobs=None, mode=None):
        # the modes rotate over the rows; `mode` overrides where a class of variants would otherwise miss one
        rows.append(Row(name, bwd, B, H, ndir, flags, variant, launches, mode or MODES[len(rows) % 4], gru, lens,
                        tuple(sorted((knobs or {}).items()))))
    F, BF = "f32", "bf"
    # forward, f32 MFMA kernel <MT, NT, KGW, DB>
    add("f_1x1_k4", 0, 3, 20, 2, (F, 1, 1, 4, 1), gru=True)                # H % 16 != 0
    add("f_1x1_k8", 0, 1, 260, 1, (F, 1, 1, 8, 1))
    add("f_1x1_k16", 0, 1, 516, 1, (F, 1, 1, 16, 1))
    add("f_1x2_k8", 0, 81, 340, 1, (F, 1, 2, 8, 1), gru=True, lens=True)
    add("f_2x1_k4", 0, 33, 172, 2, (F, 2, 1, 4, 1), gru=True)
    add("f_2x1_k8", 0, 17, 260, 2, (F, 2, 1, 8, 1))
    add("f_2x1_k16", 0, 1, 516, 2, (F, 2, 1, 16, 1), gru=True)
    add("f_2x2_k16_sb", 0, 17, 516, 2, (F, 2, 2, 16, 0), gru=True)
    add("f_4x1_k4", 0, 65, 204, 2, (F, 4, 1, 4, 1))
    add("f_4x1_k8_sb", 0, 33, 340, 2, (F, 4, 1, 8, 0), gru=True, lens=True)
    add("f_2x1_k16_launches", 0, 129, 516, 1, (F, 2, 1, 16, 1), launches=3)               # 9 batch groups as 3 + 3 + 3
    add("f_2x1_k8_short_last_launch", 0, 97, 292, 2, (F, 2, 1, 8, 1), launches=3, gru=True)     # 7 groups as 3 + 3 + 1
    # forward, bf16x6 kernel <MT, NT, DB, KSW>, and the f32 kernel forced onto a wide layer
    add("fb_2x1_k4", 0, 17, 512, 2, (BF, 2, 1, 4, 1), gru=True)
    add("fb_4x1_k8", 0, 17, 1024, 2, (BF, 4, 1, 8, 0), gru=True, lens=True)
    add("f_2x2_k16_h1024", 0, 17, 1024, 2, (F, 2, 2, 16, 0), flags=F32_MFMA)
    # backward, f32 MFMA kernel <NT, RK> with run-time UB
    add("b_16x1", 1, 3, 20, 2, (F, 16, 1, 0), gru=True)
    add("b_16x1_rk", 1, 1, 640, 1, (F, 16, 1, 32), gru=True)
    add("b_16x1_rk_ragged", 1, 1, 644, 1, (F, 16, 1, 32), mode=MODES[2])   # last k-group has 4 columns
    add("b_8x1", 1, 1, 516, 1, (F, 8, 1, 0))
    add("b_8x1_rk_ragged", 1, 1, 1156, 1, (F, 8, 1, 32))      # only past the forward's H <= 1024: the BPTT entry alone
    add("b_8x2", 1, 17, 516, 2, (F, 8, 2, 0), gru=True)
    add("b_8x4", 1, 33, 516, 2, (F, 8, 4, 0), gru=True)
    add("b_16x2", 1, 65, 404, 2, (F, 16, 2, 0), gru=True)
    add("b_16x4", 1, 129, 404, 2, (F, 16, 4, 0))
    add("b_8x1_launches", 1, 65, 516, 2, (F, 8, 1, 0), launches=5, gru=True)            # 5 batch groups, one per launch
    # backward, bf16x6 kernel
    add("bb_h512", 1, 17, 512, 2, (BF, 16, 1, 0), gru=True)
    add("bb_h1024", 1, 17, 1024, 2, (BF, 16, 1, 0))
    # variants only a tuning knob (or a device with fewer CUs) selects: run in a child process per knob set
    k = {"ASRK_FWD_MT": "1", "ASRK_FWD_NT": "4"}
    add("k_1x4_k4", 0, 50, 36, 2, (F, 1, 4, 4, 1), knobs=k, gru=True)
    add("k_1x4_k8", 0, 50, 260, 1, (F, 1, 4, 8, 1), knobs=k)
    add("k_1x4_k16", 0, 50, 516, 1, (F, 1, 4, 16, 1), knobs=k)
    k = {"ASRK_FWD_MT": "1", "ASRK_FWD_NT": "2"}
    add("k_1x2_k4", 0, 19, 36, 2, (F, 1, 2, 4, 1), knobs=k)
    add("k_1x2_k16", 0, 19, 516, 1, (F, 1, 2, 16, 1), knobs=k, gru=True)
    k = {"ASRK_FWD_MT": "2", "ASRK_FWD_NT": "2"}
    add("k_2x2_k4", 0, 19, 36, 2, (F, 2, 2, 4, 1), knobs=k)
    add("k_2x2_k8", 0, 19, 260, 2, (F, 2, 2, 8, 1), knobs=k, gru=True)
    add("kb_2x2_k4", 0, 19, 512, 2, (BF, 2, 2, 4, 1), knobs=k, gru=True)
    k = {"ASRK_REC_BF_MT4": "0"}
    add("kb_2x1_k8", 0, 16, 1024, 2, (BF, 2, 1, 8, 1), knobs=k)
    add("kb_2x2_k8_sb", 0, 33, 1024, 1, (BF, 2, 2, 8, 0), knobs=k, gru=True)
    k = {"ASRK_BWD_UB": "4"}
    add("k_b_4x1", 1, 3, 20, 2, (F, 4, 1, 0), knobs=k)
    add("k_b_4x2", 1, 17, 260, 2, (F, 4, 2, 0), knobs=k, gru=True)
    add("k_b_4x4", 1, 33, 260, 2, (F, 4, 4, 0), knobs=k)
    return rows


ROWS = _rows()
Case = namedtuple("Case", "name row kind mode")      # kind: 'lstm' | 'gru' | 'lens'


def _cases():
    out = []
    for i, r in enumerate(ROWS):
        out.append(Case(r.name, r, "lstm", r.mode))
        if r.gru:       # the GRU run takes the next mode of the rotation: more (variant, mode) pairs for the same rows
            out.append(Case(r.name + "-gru", r, "gru", MODES[(MODES.index(r.mode) + 1) % 4]))
        if r.lens:
            out.append(Case(r.name + "-lens", r, "lens", MODES[(MODES.index(r.mode) + 2) % 4]))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
PLAIN_CASES = [c for c in CASES if not c.row.knobs]
KNOB_SETS = sorted({c.row.knobs for c in CASES if c.row.knobs})


def knob_cases(knobs):
    return [c for c in CASES if c.row.knobs == knobs]


def variant_of(info, bwd):
    """the row's `variant` tuple from an asrk_lstm_plan_info record"""
    fam = "bf" if info[0] else "f32"
    if bwd:
        return (fam, info[1], info[2], info[3])
    return (fam, info[1], info[2], info[3], info[4])


def case_lens(case):
    """lengths that differ inside every 16-row batch tile and contain 1 and T"""
    return torch.tensor([1 + (5 * b) % T for b in range(case.row.B)], dtype=torch.int64)


# ------------------------------------------------------------------------------------------------ inputs, references
def _f32(x):
    return x.float().double()      # every input is an exact f32 value: the device and the float64 reference see the same


def make_inputs(case):
    """G, W_hh (per direction) and dY as float64 tensors holding f32 values; seed fixed per case"""
    r = case.row
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) & 0x7fffffff)
    gru = case.kind == "gru"
    G = torch.randn(T, r.B, r.ndir, 4, r.H, generator=g, dtype=torch.float64)
    if gru:
        G[:, :, :, 3] = torch.randn(r.ndir, r.H, generator=g, dtype=torch.float64)      # b_hn, the same in every row
    scale = min(0.4, 1.5 / r.H ** 0.5)
    whh = [_f32(torch.randn((3 if gru else 4) * r.H, r.H, generator=g, dtype=torch.float64) * scale)
           for _ in range(r.ndir)]
    mode, rate = case.mode
    dY = _f32(torch.randn(*dy_shape(mode, rate, T, r.B, r.ndir * r.H), generator=g, dtype=torch.float64))
    return _f32(G.reshape(T * r.B, r.ndir * 4 * r.H)), whh, dY


def _run(case, G, whh, dY, dtype):
    """the reference of one case in `dtype` -> dict of tensors.  Backward cases differentiate from the FLOAT64 forward
    state rounded to f32 (what the device is given), whatever `dtype` the BPTT itself runs in."""
    r = case.row
    mode, rate = case.mode
    a = (T, r.B, r.H, r.ndir)
    if not r.bwd:
        G, whh = G.to(dtype), [w.to(dtype) for w in whh]
        if case.kind == "gru":
            Y, A = gru_fwd(G, whh, *a)
            out = {"Y": Y, "gates": A}
        elif case.kind == "lens":
            Y, C, A, valid = lstm_fwd_len(G, whh, case_lens(case), *a)
            out = {"Y": Y, "C": C, "gates": A}
        else:
            Y, C, A = lstm_fwd(G, whh, *a)
            out = {"Y": Y, "C": C, "gates": A}
        if mode:
            out["Y2"] = reduce_time(Y, mode, rate, case_lens(case) if case.kind == "lens" else None)
        return out
    st = bwd_state(case)
    dYf = expand_dy(dY, mode, rate, T).to(dtype)
    whh = [w.to(dtype) for w in whh]
    if case.kind == "gru":
        dG, db = gru_bwd(st["gates"].to(dtype), whh, st["Y"].to(dtype), dYf, *a)
    else:
        dG, db = lstm_bwd(st["gates"].to(dtype), whh, st["C"].to(dtype), dYf, *a)
    return {"dG": dG, "db": db}


@functools.lru_cache(maxsize=None)
def bwd_state(case):
    """what a backward case is run ON: the float64 forward's gates / C / Y rounded to f32, so that an error of the
    device's forward can neither cause nor hide a failure of its backward"""
    r = case.row
    G, whh, _ = make_inputs(case)
    if case.kind == "gru":
        Y, A = gru_fwd(G, whh, T, r.B, r.H, r.ndir)
        return {"gates": _f32(A), "Y": _f32(Y)}
    Y, C, A = lstm_fwd(G, whh, T, r.B, r.H, r.ndir)
    return {"gates": _f32(A), "C": _f32(C)}


@functools.lru_cache(maxsize=None)
def reference(case):
    """float64 reference tensors of a case (computed once, shared, never modified)"""
    return _run(case, *make_inputs(case), torch.float64)


def rel_err(a, b):
    """SURVEY §8d metric of tests/helpers.py, in torch: max|a - b| / max|b|"""
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


@functools.lru_cache(maxsize=None)
def e32(case):
    """per tensor: error of the SAME reference run in float32 on the CPU against the float64 run"""
    ref = reference(case)
    lo = _run(case, *make_inputs(case), torch.float32)
    return {k: rel_err(lo[k], ref[k]) for k in ref}


# ------------------------------------------------------------------------------------------------ tolerance
CEILING = 1e-3                  # the project's parity bar (tests/helpers.py): never exceeded
MARGIN = 8.0                    # v_rcp_f32 / __expf are 1-2 ulp, MFMA / cross-wave summation order differs: each of the
                                # order of the reference's own f32 rounding


@functools.lru_cache(maxsize=None)
def floors():
    """per tensor kind the largest e32 over the whole table: the floor for a case whose own e32 happens to be tiny"""
    fl = {}
    for c in CASES:
        for k, v in e32(c).items():
            fl[k] = max(fl.get(k, 0.0), v)
    return fl


def bound(case, kind):
    return min(CEILING, max(MARGIN * e32(case)[kind], floors()[kind]))
