"""In-tree build of the native pieces (explicit hipcc / g++ command lines, no build system):

  lib/libhmsbeagle-jni.so   HIP engine + C ABI + JNI shim, gfx950 only   (csrc/*.hip, csrc/*.cpp)
  lib/libhmsbeagle-jni-bit.so   the natives of beagle.basta.BastaJNIWrapper: thin wrappers over the engine's beagleBasta* calls,
                            linked against the engine library next to it   (jni_basta/*.cpp, plain g++)
  lib/libmds2_jni.so        multidimensional scaling: HIP kernels + C ABI (include/mds_mi355.h) + the 14 natives of
                            dr.inference.multidimensionalscaling.NativeMDSSingleton, gfx950 only; it stands alone (no engine
                            library next to it)   (csrc/kernels_mds.hip, csrc/engine_mds.cpp, jni_mds/jni_mds.cpp)
  lib/libbeast_host.so      the caller stand-in: BeagleTreeLikelihood's call protocol in C++  (tools/host/tree_likelihood.cpp;
                            harness for tests and bench.py — in production the caller is BEAST's Java)
  lib/lab/libhmsbeagle-jni.so   (``--lab`` only) the same engine compiled with -DBEAGLE_MI355_LAB: the tuning knobs and timing
                            experiments of csrc/kernels.h labEnv() — some of which give wrong results by construction — are
                            connected to the environment ONLY in this build; select it with BEAGLE_MI355_ENGINE_LIB=<path>

hipcc cross-compiles for gfx950 without a GPU, so this runs in the build container; the built
``.so`` files travel to the GPU box with the repo snapshot.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "lib")
CSRC = os.path.join(HERE, "csrc")
HOST = os.path.join(ROOT, "tools", "host")
JNI_BASTA = os.path.join(HERE, "jni_basta")
JNI_MDS = os.path.join(HERE, "jni_mds")
MDS_SOURCES = ("kernels_mds.hip", "engine_mds.cpp")      # csrc files of libmds2_jni.so: not part of the engine library
MDS_HEADERS = ("kernels_mds.h",)


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _run(cmd):
    print("+ " + " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def build_engine(force=False, lab=False):
    """Each source is compiled to its own object (in parallel, only when it or a header changed) and the objects are
    linked into the one shared library; the 4-state kernel file alone takes minutes, the rest seconds."""
    from concurrent.futures import ThreadPoolExecutor
    lib_dir = os.path.join(LIB, "lab") if lab else LIB
    os.makedirs(lib_dir, exist_ok=True)
    obj_dir = os.path.join(lib_dir, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    out = os.path.join(lib_dir, "libhmsbeagle-jni.so")
    srcs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".cpp")) and f not in MDS_SOURCES]
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc")) and f not in MDS_HEADERS] + \
        [os.path.join(ROOT, "include", "beagle_mi355.h")]
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DBEAGLE_MI355_BUILD", "-Wall",
             "-Wno-unused-result", "-Wno-unused-value", "-Wno-cuda-compat", "-fvisibility=hidden"] + (["-DBEAGLE_MI355_LAB"] if lab else [])
    objs, jobs = [], []
    for s in srcs:
        o = os.path.join(obj_dir, os.path.basename(s) + ".o")
        objs.append(o)
        if force or _newer(o, [s] + headers):
            jobs.append([hipcc()] + flags + ["-c", "-x", "hip", s, "-o", o])
    if jobs:
        with ThreadPoolExecutor(max_workers=len(jobs)) as pool:
            list(pool.map(_run, jobs))
    # what the library exports is its interface and nothing else: the BEAGLE C API (beagle*, the engine's own beagleMi355*
    # entry points included) and the 47 JNI natives of beagle.BeagleJNIWrapper — a JNI library lives in a JVM next to other
    # natives, so planner / launcher / device-stub symbols stay local (csrc/exports.map)
    exports = os.path.join(CSRC, "exports.map")
    if jobs or force or _newer(out, objs + [exports]):
        _run([hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + objs + ["-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,/opt/rocm/lib",
             "-Wl,--version-script=" + exports, "-o", out])
    return out


def build_host(force=False):
    os.makedirs(LIB, exist_ok=True)
    out = os.path.join(LIB, "libbeast_host.so")
    src = os.path.join(HOST, "tree_likelihood.cpp")
    if force or _newer(out, [src, os.path.join(ROOT, "include", "beagle_mi355.h")]):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", src, "-o", out])
    return out


def build_basta_jni(force=False):
    """libhmsbeagle-jni-bit.so (the name BastaJNIWrapper loads): it holds no device code, finds the engine library in its own
    directory ($ORIGIN) and exports the seven natives only (jni_basta/exports.map)."""
    os.makedirs(LIB, exist_ok=True)
    out = os.path.join(LIB, "libhmsbeagle-jni-bit.so")
    engine = os.path.join(LIB, "libhmsbeagle-jni.so")
    src = os.path.join(JNI_BASTA, "jni_basta.cpp")
    exports = os.path.join(JNI_BASTA, "exports.map")
    if force or _newer(out, [src, exports, engine, os.path.join(CSRC, "jni_min.h"), os.path.join(ROOT, "include", "beagle_mi355.h")]):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-fvisibility=hidden", src, "-L" + LIB, "-l:libhmsbeagle-jni.so",
              "-Wl,-rpath,$ORIGIN", "-Wl,--no-undefined", "-Wl,--version-script=" + exports, "-o", out])
    return out


def build_mds(force=False):
    """libmds2_jni.so (the name NativeMDSSingleton loads): kernels, C ABI and natives in one library of its own.  The kernel
    file's resource report (-Rpass-analysis=kernel-resource-usage) is kept next to the library as mds_kernel_resources.txt,
    and a kernel that spills to scratch fails the build."""
    os.makedirs(LIB, exist_ok=True)
    obj_dir = os.path.join(LIB, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    out = os.path.join(LIB, "libmds2_jni.so")
    exports = os.path.join(JNI_MDS, "exports.map")
    srcs = [os.path.join(CSRC, f) for f in MDS_SOURCES] + [os.path.join(JNI_MDS, "jni_mds.cpp")]
    headers = [os.path.join(CSRC, f) for f in MDS_HEADERS + ("jni_min.h",)] + [os.path.join(ROOT, "include", "mds_mi355.h")]
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DMDS_MI355_BUILD", "-Wall", "-Wno-unused-result",
             "-Wno-cuda-compat", "-fvisibility=hidden"]
    objs, built = [], False
    for s in srcs:
        o = os.path.join(obj_dir, "mds_" + os.path.basename(s) + ".o")
        objs.append(o)
        if not (force or _newer(o, [s] + headers)):
            continue
        built = True
        if s.endswith(".hip"):
            cmd = [hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "-x", "hip", s, "-o", o]
            print("+ " + " ".join(cmd), flush=True)
            done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            report = [line for line in done.stdout.splitlines() if "remark:" in line]
            other = [line for line in done.stdout.splitlines() if "remark:" not in line and line.strip()]
            if other:
                print("\n".join(other), flush=True)
            if done.returncode:
                raise subprocess.CalledProcessError(done.returncode, cmd)
            report = [line.split("remark: ", 1)[1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").rstrip() for line in report]
            with open(os.path.join(LIB, "mds_kernel_resources.txt"), "w") as fh:
                fh.write("\n".join(report) + "\n")
            spills = [line for line in report if "ScratchSize [bytes/lane]:" in line and not line.endswith(": 0")]
            if spills:
                os.remove(o)
                raise RuntimeError("an MDS kernel uses scratch memory:\n" + "\n".join(spills))
        else:
            _run([hipcc()] + flags + ["-c", "-x", "hip", s, "-o", o])
    if built or force or _newer(out, objs + [exports]):
        _run([hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + objs + ["-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
             "-Wl,--no-undefined", "-Wl,--version-script=" + exports, "-o", out])
    return out


def build_all(force=False):
    return [build_engine(force), build_basta_jni(force), build_mds(force), build_host(force)]


if __name__ == "__main__":
    if "--lab" in sys.argv:
        print(build_engine(force="--force" in sys.argv, lab=True))
    else:
        build_all(force="--force" in sys.argv)
