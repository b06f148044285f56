"""Diagnostic hooks stay out of the shipped library (no GPU needed). IROCM_W128_DBG, IROCM_CONV32_TRACE, IROCM_CONV_TAP_TRACE and
IROCM_CONV_EPI_PROBE make a launch return wrong numbers on purpose (no stores, a trace kernel without the reduce pass, ...): they are
read through diag_getenv (csrc/diag.h), which is getenv only under -DIROCM_DIAG (tools/diag_build.py), so the shipped library does
not even hold their names. The dropped K-loop schedule variants (IROCM_KV, docs/history/gemm256p_kloop_variants.md) stay deleted."""
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
LIB = REPO / "infinitensor_amd" / "lib" / "libinfini_rocm.so"
CSRC = REPO / "infinitensor_amd" / "csrc"
DIAG_HOOKS = ("IROCM_W128_DBG", "IROCM_CONV32_TRACE", "IROCM_CONV_TAP_TRACE", "IROCM_CONV_EPI_PROBE")


@pytest.fixture(scope="module")
def lib_bytes():
    if not LIB.exists():
        pytest.skip("libinfini_rocm.so is not built")
    return LIB.read_bytes()


def test_shipped_library_holds_no_diagnostic_hook_name(lib_bytes):
    # the control: a routing hook's name IS there, so a hook the library reads would be seen
    assert b"IROCM_KVCACHE_SPLIT" in lib_bytes
    present = [h for h in DIAG_HOOKS if h.encode() in lib_bytes]
    assert not present, f"the shipped library reads diagnostic hooks: {present}"


def test_no_source_names_a_kloop_schedule_variant():
    # IROCM_KV followed by a non-identifier character: IROCM_KVCACHE_SPLIT does not match
    pat = re.compile(r"IROCM_KV(?![A-Za-z0-9_])")
    hits = [f"{f.relative_to(REPO)}:{i + 1}" for f in sorted(CSRC.rglob("*")) if f.is_file()
            for i, line in enumerate(f.read_text(errors="replace").splitlines()) if pat.search(line)]
    assert not hits, f"IROCM_KV is back in the sources: {hits}"
