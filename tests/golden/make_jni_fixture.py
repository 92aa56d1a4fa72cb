"""Writes tests/golden/jni_natives.json: name -> method descriptor of every `native` method of the reference's JNI binding
classes, lib/beagle.jar!beagle/BeagleJNIWrapper.class (key "natives") and, when the jar holds it,
beagle/basta/BastaJNIWrapper.class (key "basta_natives").

A JVM resolves Java_beagle_BeagleJNIWrapper_<name> by name and passes the arguments its descriptor lists; nothing tells it how
the C function was declared.  The fixture is what the tests hold beast-mcmc_amd/csrc/jni_shim.cpp to: the parameter lists of its
definitions (tests/test_jni_marshalling.py) and the argument types of every call the fake JNIEnv makes (tests/jni_env.py).

Names and descriptor strings only: the class file is parsed (constant pool, fields skipped, method table; methods with ACC_NATIVE
kept), no byte of it is copied.

Run from the repository root:  python tests/golden/make_jni_fixture.py [path/to/beagle.jar]
"""
import json
import os
import struct
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_JAR = "/root/reference/lib/beagle.jar"
ACC_NATIVE = 0x0100


def native_methods(data):
    """{name: descriptor} of the ACC_NATIVE methods of one class file (JVM specification, chapter 4)."""
    magic, = struct.unpack_from(">I", data, 0)
    assert magic == 0xCAFEBABE
    pos = 8
    count, = struct.unpack_from(">H", data, pos)
    pos += 2
    utf8 = {}
    i = 1
    while i < count:
        tag = data[pos]
        if tag == 1:                                        # CONSTANT_Utf8
            n, = struct.unpack_from(">H", data, pos + 1)
            utf8[i] = data[pos + 3:pos + 3 + n].decode("utf-8", "replace")
            pos += 3 + n
        elif tag in (5, 6):                                 # Long, Double: two pool slots
            pos += 9
            i += 1
        elif tag in (3, 4, 9, 10, 11, 12, 17, 18):
            pos += 5
        elif tag in (7, 8, 16, 19, 20):
            pos += 3
        elif tag == 15:                                     # MethodHandle
            pos += 4
        else:
            raise ValueError("constant pool tag %d" % tag)
        i += 1
    pos += 6                                                # access flags, this class, super class
    n_interfaces, = struct.unpack_from(">H", data, pos)
    pos += 2 + 2 * n_interfaces

    def skip_attributes(p):
        n, = struct.unpack_from(">H", data, p)
        p += 2
        for _ in range(n):
            length, = struct.unpack_from(">I", data, p + 2)
            p += 6 + length
        return p

    n_fields, = struct.unpack_from(">H", data, pos)
    pos += 2
    for _ in range(n_fields):
        pos = skip_attributes(pos + 6)
    n_methods, = struct.unpack_from(">H", data, pos)
    pos += 2
    out = {}
    for _ in range(n_methods):
        flags, name, desc = struct.unpack_from(">HHH", data, pos)
        pos = skip_attributes(pos + 6)
        if flags & ACC_NATIVE:
            assert utf8[name] not in out, "overloaded native " + utf8[name]
            out[utf8[name]] = utf8[desc]
    return out


def main():
    jar = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_JAR
    z = zipfile.ZipFile(jar)
    doc = {"source": "lib/beagle.jar!beagle/BeagleJNIWrapper.class of the reference tree: the methods with ACC_NATIVE, name -> "
                     "descriptor (tests/golden/make_jni_fixture.py)",
           "natives": native_methods(z.read("beagle/BeagleJNIWrapper.class"))}
    if "beagle/basta/BastaJNIWrapper.class" in z.namelist():
        doc["basta_natives"] = native_methods(z.read("beagle/basta/BastaJNIWrapper.class"))
    with open(os.path.join(HERE, "jni_natives.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
