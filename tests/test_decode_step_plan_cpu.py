"""CPU: every shape of the decode-step case table (tests/decode_step_reference.py) gets the energy kernel, the
softmax/context kernel and the cell branch the table names, and the table reaches everything a decode step can select -
asked of the library itself: asrk_speller_plan_info for the energy kernel, asrk_speller_ctx_variant (the function
speller_step_fwd calls, evaluated host-only) for the softmax/context kernel.  The cell branch is a predicate of
MultiSpellerStepper.step, restated in decode_step_reference.cell_branch and held to decoder_ops' threshold here.  A
re-tune that moves a case fails here instead of silently taking a kernel out of the GPU tests' reach: then move the
SHAPE back onto the variant, not the assertion."""
import ctypes
import importlib

import pytest

from conftest import PKG_NAME
import decode_step_reference as D

CTX_NAMES = {0: 'scalar', 1: 'vector', 2: 'group'}


@pytest.fixture(scope="module")
def lib():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib").load()


def descriptor(c):
    """the asrk_speller_t the stepper of this case hands to asrk_speller_step_f32, without buffers"""
    sops = importlib.import_module(PKG_NAME + ".speller_ops")
    d = sops.SpellerT(c.n, c.Te, c.A, c.Dv, c.K, (c.taps - 1) // 2, c.H, c.E, 1, D.TEMPERATURE,
                      1 if c.stepper == 'shared' else 0)
    d.cell, d.row_group = c.cell, c.rg
    return d


def selected(lib, c):
    d = descriptor(c)
    info, variant = (ctypes.c_int * 8)(), ctypes.c_int(-1)
    assert lib.asrk_speller_plan_info(ctypes.byref(d), info) == 0, c.name
    assert lib.asrk_speller_ctx_variant(ctypes.byref(d), ctypes.byref(variant)) == 0, c.name
    energy = D.STAGED if info[0] == 0 else (info[0], info[1])
    return energy, CTX_NAMES[variant.value]


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_case_gets_the_kernels_the_table_names(lib, case):
    energy, ctx = selected(lib, case)
    assert energy == case.energy
    assert ctx == case.ctx
    assert D.cell_branch(case) == case.branch


def test_cell_branch_threshold_is_the_steppers():
    dops = importlib.import_module(PKG_NAME + ".decoder_ops")
    assert dops.LSTM_CELL_GEMM_ROWS == D.LSTM_CELL_GEMM_ROWS


def test_table_reaches_every_decode_step_form(lib):
    gpu = [c for c in D.CASES if c.gpu]
    got = {c.name: selected(lib, c) for c in gpu}
    assert {v[1] for v in got.values()} == {'scalar', 'vector', 'group'}
    family = lambda c: 'staged' if got[c.name][0] == D.STAGED else 'ae2'
    # row -> memory indirection that is not the identity and not monotonic, in both energy-kernel families
    assert {family(c) for c in gpu if c.row_mem is not None} == {'staged', 'ae2'}
    assert {family(c) for c in gpu if c.stepper == 'shared'} == {'staged', 'ae2'}
    assert {D.cell_branch(c) for c in gpu} == {'fused', 'gemm'}
    # the group kernel under both cell branches and both cells, and each boundary of its dispatch from the other side
    grouped = [c for c in gpu if got[c.name][1] == 'group']
    assert {D.cell_branch(c) for c in grouped} == {'fused', 'gemm'} and {c.cell for c in grouped} == {0, 1}
    assert all(selected(lib, c)[1] != 'group' for c in D.CASES if not c.gpu)
    # the per-row kernel's query-given form (Wq == NULL) belongs to the gemm branch: at least one such case is vector
    assert any(D.cell_branch(c) == 'gemm' and got[c.name][1] == 'vector' for c in gpu)


def test_group_dispatch_boundaries(lib):
    """each condition of the group dispatch, one step on either side of it, from one base shape"""
    base = next(c for c in D.CASES if c.name == 'm_rg2_gemm')
    assert selected(lib, base)[1] == 'group'
    flips = dict(n=126, Dv=30, rg=1, stepper='shared')
    for field, value in flips.items():
        assert selected(lib, base._replace(**{field: value}))[1] != 'group', field
    big = next(c for c in D.CASES if c.name == 'm_rg32_te512')
    assert selected(lib, big)[1] == 'group'                                      # 32 rows x 512 frames = 64 KiB
    assert selected(lib, big._replace(Te=513))[1] == 'vector'                    # rounds up to 516 frames
    assert selected(lib, big._replace(rg=33, n=264))[1] == 'vector'


def test_ctx_variant_reads_alignment_from_the_pointers(lib):
    c = next(c for c in D.CASES if c.name == 'm_rg2_gemm')
    variant = ctypes.c_int(-1)
    d = descriptor(c)
    d.value = 4096 + 4                           # never dereferenced: the query runs on the host
    assert lib.asrk_speller_ctx_variant(ctypes.byref(d), ctypes.byref(variant)) == 0 and variant.value == 0
    d = descriptor(c)
    d.value, d.ctx = 4096, 4096 + 8              # a misaligned context buffer: per-row kernel, still 16-byte loads
    assert lib.asrk_speller_ctx_variant(ctypes.byref(d), ctypes.byref(variant)) == 0 and variant.value == 1
    d.ctx = 8192
    assert lib.asrk_speller_ctx_variant(ctypes.byref(d), ctypes.byref(variant)) == 0 and variant.value == 2


def test_ctx_variant_rejects_what_check_dims_rejects(lib):
    c = next(c for c in D.CASES if c.name == 'm_perm')
    variant = ctypes.c_int(-1)
    assert lib.asrk_speller_ctx_variant(ctypes.byref(descriptor(c)), None) == -1
    assert lib.asrk_speller_ctx_variant(None, ctypes.byref(variant)) == -1
    for field, value, rc in (('Te', 0, -1), ('Dv', 0, -1), ('K', 0, -1), ('temperature', 0.0, -1), ('att_mode', 2, -1),
                             ('nhead', 2, -2), ('nlayer', 4, -2), ('row_group', -1, -1)):
        d = descriptor(c)
        setattr(d, field, value)
        assert lib.asrk_speller_ctx_variant(ctypes.byref(d), ctypes.byref(variant)) == rc, field
        info = (ctypes.c_int * 8)()
        if field != 'row_group':                 # plan_info does not read row_group
            assert lib.asrk_speller_plan_info(ctypes.byref(d), info) == rc, field
    assert variant.value == -1                   # nothing was written on a refusal
