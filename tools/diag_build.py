"""The diagnostic build of libinfini_rocm.so (-DIROCM_DIAG: csrc/diag.h) for the tools that need a hook the shipped library ignores
(IROCM_W128_DBG, IROCM_CONV32_TRACE, IROCM_CONV_TAP_TRACE, IROCM_CONV_EPI_PROBE). Call use_diag_build() BEFORE importing infinitensor_amd:
it builds infinitensor_amd/lib/ab/diag.so when that is missing or older than csrc/ (tools/build_variant.py: only the translation units that
read a hook are recompiled, so run the regular build first) and points INFINI_ROCM_LIB at it.
  python tools/diag_build.py     builds it and prints the path"""
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

DIAG_LIB = REPO / "infinitensor_amd" / "lib" / "ab" / "diag.so"
# gemm128w.hip, gemm32.hip, gemm256p_conv3.hip read their hook themselves; conv.hip calls conv_route.h's conv_hooks()
DIAG_TUS = ["gemm128w.hip", "gemm32.hip", "gemm256p_conv3.hip", "conv.hip"]


def use_diag_build() -> Path:
    newest = max(f.stat().st_mtime for f in (REPO / "infinitensor_amd" / "csrc").iterdir())
    if not DIAG_LIB.exists() or DIAG_LIB.stat().st_mtime < newest:
        try:
            from tools.build_variant import build_variant

            build_variant("diag", DIAG_TUS, ["-DIROCM_DIAG"])
        except Exception as e:  # noqa: BLE001 (no compiler, a compile error: the tool cannot run either way)
            sys.exit(f"diagnostic build {DIAG_LIB} is missing or stale and could not be built (python tools/diag_build.py): {e}")
    os.environ["INFINI_ROCM_LIB"] = str(DIAG_LIB)
    return DIAG_LIB


if __name__ == "__main__":
    print(use_diag_build())
