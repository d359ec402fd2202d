"""CPU-side checks of the per-row previous-joints entry points (rsik_solve_rows, rsik_control_discrete_rows): declared,
exported, ABI version 8, and argument checks that need no device."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_entry_points_are_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    assert {"rsik_solve_rows", "rsik_control_discrete_rows"} <= set(_abi.PROTOTYPES)
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`rsik_solve_rows`" in doc and "`rsik_control_discrete_rows`" in doc


def test_rows_entry_points_refuse_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert L.rsik_solve_rows(None, 0, None, None, 0, 0, None, None, None, None, None, None, None) == _abi.RSIK_E_INVALID
    assert L.rsik_control_discrete_rows(None, 0, None, None, 0, 20, 0.0, 0, None, None, 0.7, None, None, None,
                                        None) == _abi.RSIK_E_INVALID
    assert isinstance(L.rsik_solve_rows, C._CFuncPtr)
