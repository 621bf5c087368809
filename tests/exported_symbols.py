"""The cholmod_hip_* entry points a built library exports: its defined dynamic symbols of that prefix, by `nm`.
tests/test_exported_symbols.py compares them with tests/golden/exported_symbols.json, tools/record_exported_symbols.py
writes that file."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "exported_symbols.json")
LIB_DIR = os.path.join(ROOT, "suitesparse_amd", "lib")
LIBS = ("libcholmod_amd.so", "libcholmod_amd_testhooks.so")       # the product, and the same with the test hooks
PREFIX = "cholmod_hip_"


def exported(lib):
    """sorted names of the defined dynamic symbols of LIB_DIR/lib that start with PREFIX"""
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, lib)], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.split()}
    return sorted(s for s in names if s.startswith(PREFIX))
