"""The sweep kernel's choice (ptmcmc_amd/csrc/ptm_sweep_plan.hpp) without a GPU: tests/cxx/sweep_plan_main.cc walks the cross product
of the facts the choice depends on, checks the properties the launch, the engine's preparations and the reported names rely on, and
prints every name the plan can produce; each of them must be a kernel of the gfx950 code objects that were built."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptmcmc_amd", "csrc")


def _tool(name):
    """a binutils tool from PATH, or LLVM's from beside the compiler the engine is built with"""
    import __graft_entry__ as G
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(G.HIPCC))), "lib", "llvm", "bin")
    for cand in (name, "llvm-" + name):
        p = shutil.which(cand) or shutil.which(cand, path=llvm)
        if p:
            return p
    raise RuntimeError("no %s on this machine" % name)


def code_object(obj, workdir):
    """the gfx950 code object inside a hipcc object file, as a file of its own"""
    base = os.path.join(workdir, os.path.basename(obj))
    subprocess.check_call([_tool("objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, base + ".fatbin"])
    bundler = _tool("clang-offload-bundler")
    targets = subprocess.check_output([bundler, "--type=o", "--list", "--input=" + base + ".fatbin"], text=True).split()
    gfx = [t for t in targets if t.startswith("hipv4-") and t.endswith("gfx950")]
    assert len(gfx) == 1, (obj, targets)
    subprocess.check_call([bundler, "--type=o", "--unbundle", "--targets=" + gfx[0], "--input=" + base + ".fatbin", "--output=" + base + ".co"])
    return base + ".co"


def kernels_of(code_obj):
    """the demangled kernels (defined text symbols) of a code object"""
    syms = subprocess.check_output([_tool("nm"), "--defined-only", code_obj], text=True)
    mangled = [ln.split()[2] for ln in syms.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"]
    out = subprocess.run([_tool("c++filt")], input="\n".join(mangled) + "\n", capture_output=True, text=True, check=True).stdout
    return set(out.splitlines())


def test_every_sweep_plan_names_a_kernel_that_was_built():
    import __graft_entry__ as G
    G.build_engine()
    objs = sorted(glob.glob(os.path.join(CSRC, "build", "ptm_sweep_dp*.o")))
    assert len(objs) == 9, "the per-dimension objects are missing: %s" % objs
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sweep_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "sweep_plan_main.cc"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr     # the properties, checked inside the program
        names = r.stdout.split("\n")[:-1]
        built = set()
        for o in objs:
            built |= kernels_of(code_object(o, d))
    assert len(names) > 150 and len(set(names)) == len(names)
    assert any("sweep_lanes_kernel<4, 0, true>(ptm::Dev)" in k for k in built)
    missing = []
    for n in names:
        # rocprofv3 leaves the last, defaulted argument of sweep_kernel out unless it is set
        full = n[:-1] + ", false>" if re.fullmatch(r"sweep_kernel<\d+, \d, \w+, \w+>", n) else n
        if not any(k.startswith("void ptm::%s(" % full) for k in built):
            missing.append(n)
    assert not missing, "plans that name no built kernel: %s" % missing
