"""Every GTARS_* switch the library reads is set by some test, or is listed here as a loader / process setting.

The library's kernel variants, launch shapes and recovery paths are chosen by environment switches (csrc/common.h: cfg_get).  A
variant nobody sets in tests/ is compiled, shipped and selectable, and compared with nothing: this inventory fails when such a
name appears.  A new A/B switch comes with a test that sets it (and a row in DESIGN.md section 4's table of switches)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

# Switches that select no kernel, no launch shape and no recovery path: name -> why no test sets it.
NOT_A_KERNEL_CHOICE = {
    "GTARS_AMD_LIB": "loader: the path of the shared library gtars_amd/_lib.py opens",
    "GTARS_AMD_LIB_OLDER": "loader: tolerate symbols missing from an older build loaded through GTARS_AMD_LIB (A/B tooling)",
    "GTARS_AMD_NO_TORCH": "loader: do not import torch before the library is opened",
}

QUOTED = re.compile(r'"(GTARS_[A-Z0-9_]+)"')  # as the library reads a switch: cfg_get("..."), os.environ.get("...")
TOKEN = re.compile(r"GTARS_[A-Z0-9_]+")       # whole names: GTARS_NO_LDS_PATH_FOR_TEST does not stand for GTARS_NO_LDS_PATH


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def switches_the_library_reads():
    files = [p for p in glob.glob(os.path.join(ROOT, "gtars_amd", "csrc", "*")) if os.path.isfile(p)]
    files += glob.glob(os.path.join(ROOT, "gtars_amd", "*.py"))
    return {name for p in files for name in QUOTED.findall(_read(p))}


def names_the_tests_use():
    """the test modules, the helper modules next to them and the soak fuzzers the suite loads (tests/soak) -- not this file, whose
    table would otherwise vouch for itself"""
    files = glob.glob(os.path.join(TESTS, "*.py")) + glob.glob(os.path.join(TESTS, "soak", "*.py"))
    me = os.path.abspath(__file__)
    return {name for p in files if os.path.abspath(p) != me for name in TOKEN.findall(_read(p))}


def test_every_switch_is_set_by_a_test_or_listed_as_a_process_setting():
    read = switches_the_library_reads()
    assert len(read) >= 60, sorted(read)  # (the pattern still finds the library's switches)
    used = names_the_tests_use()
    untested = sorted(read - used - set(NOT_A_KERNEL_CHOICE))
    assert not untested, "switches no test sets: " + ", ".join(untested)


def test_the_table_of_process_settings_is_current():
    read = switches_the_library_reads()
    assert all(reason.strip() for reason in NOT_A_KERNEL_CHOICE.values())
    stale = sorted(set(NOT_A_KERNEL_CHOICE) - read)
    assert not stale, "listed but no longer read by the library: " + ", ".join(stale)
    doubled = sorted(set(NOT_A_KERNEL_CHOICE) & names_the_tests_use())
    assert not doubled, "listed as untested but set by a test: " + ", ".join(doubled)
    # what the library reads through its switch snapshot (cfg_get / cfg_flag / cfg_int / env_int) can choose device code: only
    # names that Python's loader reads from os.environ may be listed
    loader = set(QUOTED.findall(_read(os.path.join(ROOT, "gtars_amd", "_lib.py"))))
    assert set(NOT_A_KERNEL_CHOICE) <= loader, sorted(set(NOT_A_KERNEL_CHOICE) - loader)
