"""Every kernel of a csrc file that takes launch geometry from grid_for / stream_grid is run past the first trip of its grid-stride
loop by a test of tests/test_gpu_grid_cap.py, or is listed here with the reason why its grid does not come from a helper.

Both helpers clip the grid far above any test shape (csrc/pipeline.h, csrc/kernels.hip), so a kernel that is wrong from its
second trip on passes every test that does not lower the cap (GTARS_GRID_CAP).  This inventory fails when a `__global__ k_*`
appears in such a file without an entry in one of the two tables: a new kernel comes with a multi-trip test, or with a reason."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gtars_amd", "csrc")
MODULE = os.path.join(ROOT, "tests", "test_gpu_grid_cap.py")

# Kernels whose grid is exact geometry computed at the launch: one workgroup per tile, per condition or per 256 items, never
# clipped, so there is no second trip to test.  kernel -> (the file that defines and launches it, why).
NOT_CAPPED = {
    "k_scan_reduce": ("kernels.hip", "one workgroup per scan tile (np tiles), tested at its tile edges by test_gpu_primitives.py"),
    "k_scan_partials": ("kernels.hip", "one workgroup walks the tile partials"),
    "k_scan_apply": ("kernels.hip", "one workgroup per scan tile"),
    "k_gather_hits": ("kernels.hip", "exactly ceil(n / 256) workgroups, no loop in the kernel"),
    "k_enum_fused": ("kernels.hip", "a persistent grid that draws tile tickets; its size is the launcher's own, not a helper's"),
    "k_occupy": ("kernels.hip", "the test hook that occupies CUs; the caller names the workgroups"),
    "k_lola_contingency": ("kernels.hip", "exactly ceil(n_files / 256) workgroups, no loop in the kernel"),
    "k_sm_tiles": ("setops.hip", "the segmented max-scan, one workgroup per 2,048-row tile (test_gpu_primitives.py)"),
    "k_sm_carry": ("setops.hip", "one workgroup walks the tile aggregates"),
    "k_sm_apply": ("setops.hip", "one workgroup per tile"),
    "k_pair_inter": ("setops.hip", "one workgroup per pair of sets and chromosome slice, indexed by blockIdx alone"),
    "k_t2_tiles": ("setops.hip", "the top-2 scan of bulk_union_except, one workgroup per 2,048-row tile (test_gpu_setlist.py)"),
    "k_t2_carry": ("setops.hip", "one workgroup walks the tile aggregates"),
    "k_t2_apply": ("setops.hip", "one workgroup per tile"),
    "k_ue_emit": ("setops.hip", "one workgroup per tile, its counts laid out by tile number"),
    "k_signal_stats": ("signal.hip", "one workgroup per condition, indexed by blockIdx alone"),
}

HELPER = re.compile(r"\b(?:grid_for|stream_grid)\s*\(")
# `__global__`, then attributes and `void` in any order, then the kernel's name in front of its parameter list
KERNEL = re.compile(r"__global__\b[^;{}]*?\b(k_\w+)\s*\(")


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def kernels_of_files_that_use_a_helper():
    """kernel name -> the files that define it, over the csrc files that call grid_for or stream_grid"""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        text = _read(path) if os.path.isfile(path) else ""
        if not HELPER.search(text):
            continue
        assert text.count("__global__") == len(KERNEL.findall(text)) or os.path.basename(path) == "pipeline.h", path  # (the pattern sees all)
        for name in KERNEL.findall(text):
            found.setdefault(name, []).append(os.path.basename(path))
    return found


def module_tables():
    """(COVERED of the GPU module, the names of its test functions), read from its text: importing it needs the library"""
    tree = ast.parse(_read(MODULE))
    covered = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERED" for t in node.targets):
            covered = ast.literal_eval(node.value)
    tests = {node.name for node in tree.body if isinstance(node, ast.FunctionDef) and node.name.startswith("test_")}
    return covered, tests


def test_every_kernel_has_a_multi_trip_test_or_a_reason():
    kernels = kernels_of_files_that_use_a_helper()
    assert len(kernels) >= 100, sorted(kernels)  # (the pattern still finds the kernels)
    covered, tests = module_tables()
    assert covered, "tests/test_gpu_grid_cap.py has no COVERED table"
    both = sorted(set(covered) & set(NOT_CAPPED))
    assert not both, "in both tables: " + ", ".join(both)
    missing = sorted(set(kernels) - set(covered) - set(NOT_CAPPED))
    assert not missing, "kernels without a multi-trip test or a reason: " + ", ".join(f"{k} ({', '.join(kernels[k])})" for k in missing)
    no_such_test = sorted(k for k, t in covered.items() if t not in tests)
    assert not no_such_test, "COVERED names a test that does not exist: " + ", ".join(f"{k} -> {covered[k]}" for k in no_such_test)


def test_the_tables_are_current():
    kernels = kernels_of_files_that_use_a_helper()
    covered, _ = module_tables()
    stale = sorted((set(covered) | set(NOT_CAPPED)) - set(kernels))
    assert not stale, "listed but no longer defined in a file that uses a helper: " + ", ".join(stale)
    assert all(reason.strip() for _, reason in NOT_CAPPED.values())
    assert all(name in kernels and kernels[name] == [file] for name, (file, _) in NOT_CAPPED.items())


def launches(text):
    """(kernel, grid argument, position) of every hipLaunchKernelGGL in the text: the arguments split at the commas outside brackets (a
    kernel with several template arguments stands in parentheses, or the macro would not take it)"""
    for m in re.finditer(r"hipLaunchKernelGGL\s*\(", text):
        args, depth, at = [], 0, m.end()
        for k in range(m.end(), len(text)):
            ch = text[k]
            if ch in "([{":
                depth += 1
            elif ch in ")]}":
                if depth == 0:
                    args.append(text[at:k])
                    break
                depth -= 1
            elif ch == "," and depth == 0:
                args.append(text[at:k])
                at = k + 1
        name = re.search(r"k_\w+", args[0])
        if name and len(args) > 1:
            yield name.group(0), args[1], m.start()


def through_a_helper(text, grid, at):
    """the grid argument of the launch at `at` names a helper, or a local whose nearest declaration above the launch --
    `const unsigned grid = grid_for(...)`, `const dim3 grid(grid_for(...))`, `grid{...}` -- holds a helper's answer"""
    if HELPER.search(grid):
        return True
    for word in set(re.findall(r"[A-Za-z_]\w*", grid)) - {"dim3", "unsigned"}:
        decl = re.findall(r"\b(?:unsigned|int|u32|u64|size_t|auto|dim3)\s+%s\s*[=({]([^;]*);" % word, text[:at])
        if decl and HELPER.search(decl[-1]):
            return True
    return False


def test_the_launch_reader_sees_a_helper_behind_a_local():
    text = """
        const unsigned grid = grid_for(n, HG_TPB, HG_MAX_BLOCKS);
        hipLaunchKernelGGL(k_a, dim3(grid), dim3(HG_TPB), 0, st, p, n);
        hipLaunchKernelGGL((k_b<MODE, true>), dim3(grid_for(A.n)), dim3(256), 0, st, p);
        const dim3 geometry(stream_grid(nq, 256)), block(256);
        hipLaunchKernelGGL(k_c<4>, geometry, block, 0, st, p);
        hipLaunchKernelGGL(k_d, dim3((unsigned)tiles), dim3(SO_TPB), 0, st, p);
    """
    text += """
        const unsigned grid = (unsigned)std::min<u64>(tiles, 8 * cus);
        hipLaunchKernelGGL(k_e, dim3(grid), dim3(256), 0, st, p);
    """
    got = {name: through_a_helper(text, grid, at) for name, grid, at in launches(text)}
    assert got == {"k_a": True, "k_b": True, "k_c": True, "k_d": False, "k_e": False}


def test_not_capped_kernels_are_not_launched_through_a_helper():
    """the grid argument of every launch of a NOT_CAPPED kernel names neither a helper nor a local that holds a helper's answer"""
    seen = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        text = _read(path) if os.path.isfile(path) else ""
        for name, grid, at in launches(text):
            if name in NOT_CAPPED and os.path.basename(path) == NOT_CAPPED[name][0]:
                seen.add(name)
                assert not through_a_helper(text, grid, at), (os.path.basename(path), name, grid)
    assert seen == set(NOT_CAPPED), sorted(set(NOT_CAPPED) - seen)  # (the reader still finds the launches)
