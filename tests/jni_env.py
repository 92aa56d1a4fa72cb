"""A JNIEnv in Python, for calling the Java_beagle_BeagleJNIWrapper_* natives of beast-mcmc_amd/csrc/jni_shim.cpp the way a JVM
does — without a JVM, in the test process itself.

A JNIEnv* points to a pointer to the JVM's function table (JNI specification, "Interface Function Table": 229 entries in JNI
1.6, 0-3 reserved).  `JniEnv` builds that table out of ctypes callbacks:

  slot 167 NewStringUTF, 171 GetArrayLength, 203 GetIntArrayRegion, 206 GetDoubleArrayRegion, 211 SetIntArrayRegion,
  214 SetDoubleArrayRegion                      over numpy arrays registered as "Java arrays" (handle -> array, the array's real
                                                length; a region outside it is recorded as a problem, as the JVM would throw)
  every other slot                              RECORDS ITS NUMBER in `traps` and returns zero (no abort in a process that may
                                                hold the GPU) — every test ends with `assert_clean()`

The slot numbers are written down from the specification, independently of csrc/jni_min.h (as tests/native/fake_jvm.cpp does).
`log` holds what crossed during the last call: (direction, array, start, length) with direction "get" (Java -> native) or "set".

`call(name, *args)` derives the C argument types FROM THE CLASS FILE'S DESCRIPTOR (tests/golden/jni_natives.json), not from the
shim's source: a JVM passes what the descriptor says, so a shim parameter list that disagrees with it receives its arguments in
the wrong registers and the results show it.

`JniLibrary` is the interface beagle.Beagle needs from an engine library (`fn[name]`, `version`, `partition_api_table`), with
every `fn` entry forwarding to the native of that name.  beagle.Beagle passes `array.ctypes.data_as(...)` pointers; numpy keeps
the array on such a pointer (`ptr._arr`), which is the Java array and its length.  So Beagle, gradient.BranchGradient and
multipartition.MultiPartitionTreeLikelihood(native_sequence=False) run their call sequences through the shim unchanged.
"""
import ctypes as C
import functools
import json
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PREFIX = "Java_beagle_BeagleJNIWrapper_"
TABLE_SIZE = 229
SLOT_NewStringUTF, SLOT_GetArrayLength = 167, 171
SLOT_GetIntArrayRegion, SLOT_GetDoubleArrayRegion, SLOT_SetIntArrayRegion, SLOT_SetDoubleArrayRegion = 203, 206, 211, 214


@functools.lru_cache(maxsize=None)
def natives():
    """name -> descriptor of the 47 native methods of beagle.BeagleJNIWrapper (the fixture)."""
    with open(os.path.join(GOLDEN, "jni_natives.json")) as fh:
        return json.load(fh)["natives"]


def parse_descriptor(desc):
    """'(II[D)I' -> (['I', 'I', '[D'], 'I'); object types keep their class: 'Lbeagle/InstanceDetails;'."""
    m = re.fullmatch(r"\((.*)\)(.+)", desc)
    params = re.findall(r"\[*(?:[IJDZBCSF]|L[^;]+;)", m.group(1))
    assert "".join(params) == m.group(1), desc
    return params, m.group(2)


_SCALAR = {"I": C.c_int, "J": C.c_longlong, "D": C.c_double}
_DTYPE = {"[I": np.int32, "[D": np.float64}


class JniEnv:
    def __init__(self):
        self.traps = []              # slots called that this environment does not implement
        self.problems = []           # what a JVM would have thrown for: unknown handle, wrong element type, region out of bounds
        self.log = []                # (direction, array, start, length) of the region calls of the last call()
        self.arrays = {}             # handle -> 1-D numpy array
        self.strings = {}            # handle -> str (NewStringUTF)
        self._next = 0x10000
        self._keep = []
        self._table = (C.c_void_p * TABLE_SIZE)()
        for slot in range(TABLE_SIZE):
            self._install(slot, C.CFUNCTYPE(C.c_void_p, C.c_void_p), self._trap(slot))
        self._install(SLOT_NewStringUTF, C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_char_p), self._new_string)
        self._install(SLOT_GetArrayLength, C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p), self._length)
        region = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p)
        self._install(SLOT_GetIntArrayRegion, region, self._region("get", np.int32))
        self._install(SLOT_GetDoubleArrayRegion, region, self._region("get", np.float64))
        self._install(SLOT_SetIntArrayRegion, region, self._region("set", np.int32))
        self._install(SLOT_SetDoubleArrayRegion, region, self._region("set", np.float64))
        self._table_ptr = C.c_void_p(C.addressof(self._table))          # JNIEnv = pointer to the table; JNIEnv* = &that
        self.env = C.c_void_p(C.addressof(self._table_ptr))
        self.this = C.c_void_p(self._handle())                          # the BeagleJNIWrapper object (never looked at)

    # -- the table ---------------------------------------------------------------------------------------------
    def _install(self, slot, proto, fn):
        cb = proto(fn)
        self._keep.append(cb)
        self._table[slot] = C.cast(cb, C.c_void_p).value

    def _trap(self, slot):
        def trap(env):
            self.traps.append(slot)
            return 0
        return trap

    def _handle(self):
        self._next += 16
        return self._next

    def _new_string(self, env, text):
        h = self._handle()
        self.strings[h] = (text or b"").decode()
        return h

    def _length(self, env, handle):
        a = self.arrays.get(handle)
        if a is None:
            self.problems.append("GetArrayLength of unknown handle %r" % (handle,))
            return 0
        return int(a.size)

    def _region(self, direction, dtype):
        def region(env, handle, start, length, buf):
            a = self.arrays.get(handle)
            if a is None or a.dtype != dtype:
                self.problems.append("%s region (%s) of %s" % (direction, np.dtype(dtype).name, "unknown handle" if a is None else a.dtype.name + " array"))
                return
            if start < 0 or length < 0 or start + length > a.size:                 # ArrayIndexOutOfBoundsException
                self.problems.append("%s region [%d, %d) of an array of %d" % (direction, start, start + length, a.size))
                return
            self.log.append((direction, a, int(start), int(length)))
            nbytes = length * a.itemsize
            if nbytes:
                if direction == "get":
                    C.memmove(buf, a.ctypes.data + start * a.itemsize, nbytes)
                else:
                    C.memmove(a.ctypes.data + start * a.itemsize, buf, nbytes)
        return region

    # -- Java arrays -------------------------------------------------------------------------------------------
    def register(self, array):
        """A numpy array as a Java array: -> handle.  The array itself is registered (no copy): what the native sets is seen."""
        if not (isinstance(array, np.ndarray) and array.flags.c_contiguous):
            raise TypeError("a Java array is a C-contiguous numpy array")
        h = self._handle()
        self.arrays[h] = array.reshape(-1)
        return h

    def moved(self, array, direction=None):
        """[(direction, start, length)] of the last call's region calls on `array` (optionally of one direction)."""
        flat = array.reshape(-1)
        return [(d, s, n) for d, a, s, n in self.log
                if a.ctypes.data == flat.ctypes.data and a.size == flat.size and (direction is None or d == direction)]

    def assert_clean(self):
        assert self.traps == [], "JNI slots outside the environment were called: %r" % (self.traps,)
        assert self.problems == [], self.problems

    # -- calls -------------------------------------------------------------------------------------------------
    def call(self, library, name, *args):
        """Java_beagle_BeagleJNIWrapper_<name>(env, this, *args) in `library` (a ctypes.CDLL), argument types by the descriptor.
        Arrays: numpy arrays (int32 for [I, float64 for [D) or None for null; objects: None.  A String result comes back as str."""
        params, ret = parse_descriptor(natives()[name])
        if len(args) != len(params):
            raise TypeError("%s%s takes %d arguments, %d given" % (name, natives()[name], len(params), len(args)))
        f = getattr(library, PREFIX + name)
        argtypes, values, handles = [C.c_void_p, C.c_void_p], [self.env, self.this], []
        for kind, v in zip(params, args):
            if kind in _SCALAR:
                argtypes.append(_SCALAR[kind])
                values.append(v)
                continue
            argtypes.append(C.c_void_p)
            if v is None:
                values.append(None)
            elif kind in _DTYPE:
                if not isinstance(v, np.ndarray) or v.dtype != _DTYPE[kind]:
                    raise TypeError("%s: a %s parameter takes a %s array or None" % (name, kind, np.dtype(_DTYPE[kind]).name))
                handles.append(self.register(v))
                values.append(handles[-1])
            else:
                raise TypeError("%s: only null can be passed for %s" % (name, kind))
        f.argtypes = argtypes
        f.restype = _SCALAR.get(ret, C.c_void_p)
        del self.log[:]
        try:
            out = f(*values)
        finally:
            for h in handles:
                del self.arrays[h]
        if ret == "Ljava/lang/String;":
            return self.strings.pop(out, None)
        return out


def _java_array(arg):
    """What beagle.py and its drivers hand a C function, as the Java array a JVM caller would hold."""
    if arg is None or isinstance(arg, (int, float, np.integer, np.floating)):
        return arg
    if isinstance(arg, np.ndarray):
        return arg
    arr = getattr(arg, "_arr", None)                      # ndarray.ctypes.data_as(...) keeps its array
    if isinstance(arr, np.ndarray):
        return arr
    if isinstance(arg, C.Array):                          # (c_int * n)(...): a view of the same memory
        return np.ctypeslib.as_array(arg)
    raise TypeError("cannot tell which array %r points into" % (arg,))


class JniLibrary:
    """An engine library as beagle.Beagle sees one, every call of it made through the JNI natives of `cdll`."""

    def __init__(self, engine_library, env=None):
        """engine_library: the beagle.EngineLibrary whose shared object also holds the natives."""
        self.env = env or JniEnv()
        self.engine = engine_library
        self.lib = engine_library.lib            # beagle.Beagle reaches the beagleMi355* diagnostics through it: not natives
        self.path, self.prefix = engine_library.path, ""
        self.partition_api_table = None          # (no native call sequence in C++ through this library)
        self.api_table = None
        self.called = set()
        self.fn = {}
        for name in natives():
            if name in ("getVersion", "getCitation", "getResourceList", "getBenchmarkedResourceList", "calculateEdgeDerivative"):
                continue
            key = "FinalizeInstance" if name == "finalize" else name[0].upper() + name[1:]
            self.fn[key] = self._forward(name)
        self.version = self.call("getVersion")

    def has(self, name):
        return name in self.fn

    def call(self, name, *args):
        self.called.add(name)
        return self.env.call(self.lib, name, *args)

    def _forward(self, name):
        def forward(*args):
            if name == "createInstance":                  # InstanceDetails: null (its setters are variadic JNI calls: fake_jvm.cpp)
                args = args[:-1] + (None,)
            return self.call(name, *[_java_array(a) for a in args])
        return forward
