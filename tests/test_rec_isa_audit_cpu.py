"""CPU: the parser of tools/rec_isa_audit.py on two small hand-written assembly snippets - no hipcc, no GPU.

CLEAN is a time-step loop whose fast path feeds one MFMA from an AGPR operand inside an inline-assembly statement;
DIRTY has one v_readlane_b32 and one compiler v_accvgpr_read_b32 between the two MFMAs of its loop, and metadata with a
VGPR spill and scratch.  The set-up and the slow-path block (a shorter MFMA run behind a label) must stay out of the
fast-path span; an AGPR copy inside ;;#ASMSTART / ;;#ASMEND is the author's and is not counted as the compiler's."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("rec_isa_audit", os.path.join(ROOT, "tools", "rec_isa_audit.py"))
audit = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(audit)

FWD = "_ZN8asrk_rec12_GLOBAL__N_122lstm_rec_fwd_bf_kernelILi4ELi1ELb0ELb0ELi8EEEvNS_10RecFwdArgsE"
BWD = "_ZN8asrk_rec12_GLOBAL__N_122lstm_rec_bwd_bf_kernelILb0ELi32ELi21EEEvNS_10RecBwdArgsE"

_META = """\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     %(agpr)d
    .args:
      - .offset:         0
        .size:           8
        .value_kind:     by_value
    .name:           %(name)s
    .private_segment_fixed_size: %(scratch)d
    .sgpr_count:     106
    .sgpr_spill_count: %(sspill)d
    .vgpr_count:     %(vgpr)d
    .vgpr_spill_count: %(vspill)d
    .wavefront_size: 64
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
...
\t.end_amdgpu_metadata
"""

CLEAN = """\t.text
%(name)s: ; @%(name)s
; %%bb.0:
\tv_accvgpr_write_b32 a0, v9
\tv_readlane_b32 s4, v255, 0
.LBB0_1:                                ; =>This Loop Header: Depth=1
\tbuffer_load_dwordx4 v[4:7], v8, s[0:3], 0 offen
\ts_waitcnt vmcnt(0)
\t;;#ASMSTART
\tv_mfma_f32_16x16x32_bf16 v[0:3], a[0:3], v[4:7], v[0:3]
\t;;#ASMEND
\tds_read_b128 v[10:13], v14
\t;;#ASMSTART
\tv_accvgpr_read_b32 v20, a4
\t;;#ASMEND
\ts_waitcnt lgkmcnt(0)
\tv_mfma_f32_16x16x32_bf16 v[0:3], v[10:13], v[4:7], v[0:3]
\tv_mfma_f32_16x16x32_bf16 v[0:3], v[10:13], v[4:7], v[0:3]
\ts_cbranch_execz .LBB0_3
.LBB0_2:                                ; slow path
\tv_accvgpr_read_b32 v16, a0
\tv_mfma_f32_16x16x32_bf16 v[0:3], v[16:19], v[4:7], v[0:3]
.LBB0_3:
\ts_add_i32 s5, s5, 1
\ts_cmp_lt_i32 s5, s6
\ts_cbranch_scc1 .LBB0_1
; %%bb.4:
\ts_endpgm
.Lfunc_end0:
\t.size\t%(name)s, .Lfunc_end0-%(name)s
""" % dict(name=FWD) + _META % dict(name=FWD, agpr=4, vgpr=24, scratch=0, sspill=3, vspill=0)

DIRTY = """\t.text
%(name)s: ; @%(name)s
; %%bb.0:
\tv_writelane_b32 v255, s4, 0
.LBB1_1:                                ; =>This Loop Header: Depth=1
\tv_accvgpr_read_b32 v30, a9
\tv_mfma_f32_16x16x32_bf16 v[0:3], v[10:13], v[4:7], v[0:3]
\tv_readlane_b32 s4, v255, 0
\ts_nop 4
\tbuffer_load_dwordx4 v[4:7], v8, s[0:3], s4 offen
\tv_accvgpr_read_b32 v10, a0
\ts_waitcnt vmcnt(0)
\tv_mfma_f32_16x16x32_bf16 v[0:3], v[10:13], v[4:7], v[0:3]
\tv_readlane_b32 s7, v255, 1
\ts_add_i32 s5, s5, 1
\ts_cmp_lt_i32 s5, s6
\ts_cbranch_scc1 .LBB1_1
; %%bb.2:
\ts_endpgm
.Lfunc_end1:
\t.size\t%(name)s, .Lfunc_end1-%(name)s
""" % dict(name=BWD) + _META % dict(name=BWD, agpr=206, vgpr=462, scratch=100, sspill=154, vspill=24)

OTHER = CLEAN.replace("lstm_rec_fwd_bf_kernel", "lstm_rec_fwd_f32_kernel")


def test_clean_snippet_passes():
    ks = audit.parse(CLEAN)
    assert [k.name for k in ks] == ["lstm_rec_fwd_bf_kernel<4,1,false,false,8>"]
    k = ks[0]
    assert k.meta == dict(agpr_count=4, vgpr_count=24, sgpr_count=106, sgpr_spill_count=3, vgpr_spill_count=0,
                          private_segment_fixed_size=0)
    # span: first to third MFMA of the loop's longest straight run; the slow-path MFMA behind .LBB0_2 is outside
    assert k.span["v_mfma"] == 3 and k.span_len == 6
    assert k.span["ds_read_b128"] == 1 and k.span["s_waitcnt"] == 1
    assert k.span["v_accvgpr_read_b32"] == 1 and k.span_compiler_accread == 0      # the one inside the asm statement
    assert k.span_readlane == 0
    # loop: everything from .LBB0_1 to the back edge, the set-up's AGPR write and lane read excluded
    assert k.loop["v_mfma"] == 4 and k.loop["v_accvgpr_read_b32"] == 2
    assert k.loop["v_accvgpr_write_b32"] == 0 and k.loop["v_readlane_b32"] == 0
    assert k.loop_len == 14
    assert k.violations() == []
    text, status = audit.audit_text(CLEAN)
    assert status == 0 and "verdict: ok" in text and "1 kernels, 0 failing" in text


def test_dirty_snippet_fails_with_counts():
    ks = audit.parse(DIRTY)
    assert [k.name for k in ks] == ["lstm_rec_bwd_bf_kernel<false,32,21>"]
    k = ks[0]
    assert k.span["v_mfma"] == 2 and k.span_len == 7
    assert k.span_readlane == 1 and k.span_compiler_accread == 1
    assert k.span["s_nop"] == 1 and k.span["buffer_load_dwordx4"] == 1
    # the copy in front of the first MFMA and the lane read behind the last one are in the loop, not in the span
    assert k.loop["v_readlane_b32"] == 2 and k.loop["v_accvgpr_read_b32"] == 2 and k.loop_len == 12
    assert k.meta["vgpr_spill_count"] == 24 and k.meta["private_segment_fixed_size"] == 100
    assert k.meta["sgpr_spill_count"] == 154 and k.meta["agpr_count"] == 206 and k.meta["vgpr_count"] == 462
    v = k.violations()
    assert len(v) == 4 and "24 VGPR spills" in v[0] and "100 B scratch" in v[1]
    assert v[2].startswith("1 v_readlane_b32") and v[3].startswith("1 compiler v_accvgpr_read_b32")
    text, status = audit.audit_text(DIRTY)
    assert status == 1 and "FAIL" in text and "1 kernels, 1 failing" in text


def test_both_units_together_and_foreign_kernels():
    text, status = audit.report(audit.parse(CLEAN) + audit.parse(DIRTY))
    assert status == 1 and "2 kernels, 1 failing" in text
    assert audit.parse(OTHER) == []                     # not a bf16x6 recurrence kernel: not audited
    assert audit.audit_text(OTHER)[1] == 1              # nothing found is not a pass
