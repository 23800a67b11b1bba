"""The whole ctypes binding against include/pbr_hip.h, on the host (no device): every prototype against the function objects of the loaded
library, every struct against a C compiler's sizeof / offsetof, every constant against the header's value -- and the comparisons
themselves against altered copies, so that each kind of difference is seen to be reported.  An entry point is added by writing its
prototype into the header and its row into _native.SIGNATURES; this file needs no edit for it."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import abi_header as H
from pypbr_amd import _native as N

SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
# header constants the binding does not mirror under the same name: the ABI version is N.ABI_VERSION, the two retired knob slots are private
UNMIRRORED = {"PBR_HIP_ABI_VERSION", "PBR_TUNE_RESERVED_0", "PBR_TUNE_RESERVED_4"}
XCD_ARGUMENTS = (1, 12)                  # PBR_SCHEDULE_XCD(c) is compared through N.schedule_xcd at these two


def allowed(c_type, structs):
    """The ctypes types that bind a parameter (or a result) of this C type."""
    if c_type == "void":
        return (None,)
    if c_type == "char *":
        return (ctypes.c_char_p,)
    if c_type in SCALARS:
        return (SCALARS[c_type],)
    assert c_type.endswith(" *"), c_type
    target = c_type[:-2]
    if target.startswith("pbr_"):
        return (ctypes.POINTER(structs[target]),)                    # ... and nothing else
    if target == "void":
        return (ctypes.c_void_p,)
    if target == "void *":
        return (ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p)
    return (ctypes.POINTER(SCALARS[target]), ctypes.c_void_p)        # a host array, or a device pointer


def prototype_differences(prototypes, bound, structs):
    """`bound`: {name: (restype, argtypes)}.  One line per difference, each beginning with the name it is about."""
    diffs = ["%s: declared, not bound" % n for n in sorted(set(prototypes) - set(bound))]
    diffs += ["%s: bound, not declared" % n for n in sorted(set(bound) - set(prototypes))]
    for name in sorted(set(prototypes) & set(bound)):
        (c_ret, c_args), (restype, argtypes) = prototypes[name], bound[name]
        if not any(restype is t for t in allowed(c_ret, structs)):
            diffs.append("%s: returns %s, bound as %r" % (name, c_ret, restype))
        if argtypes is None or len(argtypes) != len(c_args):
            diffs.append("%s: %d arguments, %s bound" % (name, len(c_args), "none" if argtypes is None else len(argtypes)))
            continue
        for i, (c_arg, t) in enumerate(zip(c_args, argtypes)):
            if not any(t is a for a in allowed(c_arg, structs)):
                diffs.append("%s: argument %d is %s, bound as %r" % (name, i, c_arg, t))
    return diffs


def header_structs():
    return set(re.findall(r"\}\s*(pbr_[a-z0-9_]+)\s*;", H.TEXT))


def header_constants():
    """The names of every `#define PBR_<NAME> <value>` (macros with an argument and the include guard have none) and every enumerator."""
    names = re.findall(r"^[ \t]*#define[ \t]+(PBR_[A-Z0-9_]+)[ \t]+\S", H.TEXT, flags=re.M)
    for body in re.findall(r"\benum\s*\{([^}]*)\}", H.TEXT):
        names += [re.match(r"\s*(PBR_[A-Z0-9_]+)\b", e).group(1) for e in body.split(",") if e.strip()]
    assert len(names) == len(set(names))
    return names


def c_program(structs, constants):
    """C source that prints what the compiler makes of the header: `struct <name> <sizeof>`, `field <struct> <field> <offsetof> <size>`
    for every _fields_ entry, `const <name> <value>`, `xcd <c> <PBR_SCHEDULE_XCD(c)>`."""
    out = ['#include <stdio.h>', '#include <stddef.h>', '#include "pbr_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        out.append('    printf("struct %s %%zu\\n", sizeof(%s));' % (name, name))
        for field in cls._fields_:
            out.append('    printf("field %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));'
                       % (name, field[0], name, field[0], name, field[0]))
    for name in constants:
        out.append('    printf("const %s %%lld\\n", (long long)(%s));' % (name, name))
    for c in XCD_ARGUMENTS:
        out.append('    printf("xcd %d %%lld\\n", (long long)PBR_SCHEDULE_XCD(%d));' % (c, c))
    return "\n".join(out + ['    return 0;', '}', ''])


def host_compiler():
    """The first that exists of $CC, cc, gcc, clang and the clang beside the hipcc the Makefile uses."""
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", open(os.path.join(H.ROOT, "pypbr_amd", "csrc", "Makefile")).read(),
                                                 flags=re.M).group(1)
    bin_dir = os.path.dirname(os.path.realpath(shutil.which(hipcc) or hipcc))
    beside = [os.path.join(bin_dir, "clang"), os.path.join(os.path.dirname(bin_dir), "llvm", "bin", "clang")]
    for candidate in [os.environ.get("CC"), "cc", "gcc", "clang"] + beside:
        path = candidate and shutil.which(candidate.split()[0])
        if path:
            return [path] + candidate.split()[1:]
    pytest.fail("no host C compiler (tried $CC, cc, gcc, clang, %s): the library cannot be built without one" % ", ".join(beside))


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """What the C compiler says: ({struct: (sizeof, {field: (offset, size)})}, {constant: value}, {c: PBR_SCHEDULE_XCD(c)})."""
    tmp = tmp_path_factory.mktemp("abi")
    source, program = tmp / "abi_layout.c", tmp / "abi_layout"
    source.write_text(c_program(N.STRUCTS, header_constants()))
    build = subprocess.run(host_compiler() + ["-std=c11", "-I", os.path.dirname(H.PATH), str(source), "-o", str(program)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr           # a ctypes field the header lacks stops here
    layouts, constants, xcd = {}, {}, {}
    for line in subprocess.run([str(program)], capture_output=True, text=True, check=True).stdout.splitlines():
        kind, *rest = line.split()
        if kind == "struct":
            layouts[rest[0]] = (int(rest[1]), {})
        elif kind == "field":
            layouts[rest[0]][1][rest[1]] = (int(rest[2]), int(rest[3]))
        elif kind == "const":
            constants[rest[0]] = int(rest[1])
        else:
            xcd[int(rest[0])] = int(rest[1])
    return layouts, constants, xcd


def layout_differences(layouts, structs):
    """One line per difference between the compiler's layouts and the ctypes classes, each beginning with `<struct>` or `<struct>.<field>`."""
    diffs = []
    for name, cls in structs.items():
        size, fields = layouts[name]
        if ctypes.sizeof(cls) != size:
            diffs.append("%s: %d bytes, binding %d" % (name, size, ctypes.sizeof(cls)))
        for field in cls._fields_:
            mirror = getattr(cls, field[0])
            if (mirror.offset, mirror.size) != fields[field[0]]:
                diffs.append("%s.%s: offset %d size %d, binding %d and %d" % ((name, field[0]) + fields[field[0]] + (mirror.offset, mirror.size)))
    return diffs


def constant_differences(constants, mirror):
    """`mirror`: {name without PBR_: value}.  (the lines of the mirrored constants whose values differ, the header names without a mirror)"""
    diffs = ["%s: %d, binding %d" % (name, value, mirror[name[4:]]) for name, value in constants.items()
             if name[4:] in mirror and mirror[name[4:]] != value]
    return diffs, {name for name in constants if name[4:] not in mirror}


def native_integers():
    return {k: v for k, v in vars(N).items() if isinstance(v, int) and not isinstance(v, bool) and not k.startswith("_")}


def test_every_prototype_is_bound_as_the_header_declares_it():
    lib = N.lib()
    assert set(H.PROTOTYPES) == set(N.EXPORTS) == set(re.findall(r"\b(pbr_[a-z0-9_]+)\s*\(", H.TEXT)) and len(N.EXPORTS) == len(set(N.EXPORTS))
    assert isinstance(N.EXPORTS, tuple) and N.EXPORTS == tuple(N.SIGNATURES)
    bound = {name: (getattr(lib, name).restype, getattr(lib, name).argtypes) for name in N.EXPORTS}
    assert prototype_differences(H.PROTOTYPES, bound, N.STRUCTS) == []
    print("%d prototypes, %d arguments" % (len(H.PROTOTYPES), sum(len(a) for _, a in H.PROTOTYPES.values())))


def test_every_struct_has_the_compilers_layout(compiled):
    layouts = compiled[0]
    assert header_structs() == set(N.STRUCTS) == set(layouts)
    assert layout_differences(layouts, N.STRUCTS) == []
    assert all(len(fields) == len(N.STRUCTS[name]._fields_) for name, (_, fields) in layouts.items())
    print("%d structs, %d fields" % (len(layouts), sum(len(f) for _, f in layouts.values())))


def test_every_mirrored_constant_has_the_headers_value(compiled):
    _, constants, xcd = compiled
    diffs, unmirrored = constant_differences(constants, native_integers())
    assert diffs == [] and unmirrored == UNMIRRORED
    assert constants["PBR_HIP_ABI_VERSION"] == N.ABI_VERSION and constants["PBR_TUNE_UNSET"] == N.TUNE_UNSET
    assert set(xcd) == set(XCD_ARGUMENTS) and all(N.schedule_xcd(c) == value for c, value in xcd.items())
    print("%d mirrored constants, %d without a mirror: %s" % (len(constants) - len(unmirrored), len(unmirrored), ", ".join(sorted(unmirrored))))


def test_the_comparisons_report_each_kind_of_difference(compiled):
    """Altered copies of the table, of a class and of the constants: nothing here is applied to the library or called."""
    layouts, constants, _ = compiled
    table = {name: (restype, list(argtypes)) for name, (restype, argtypes) in N.SIGNATURES.items()}
    assert prototype_differences(H.PROTOTYPES, table, N.STRUCTS) == []

    name = "pbr_blend_gradient_mask"                                  # (void *mask, int32_t height, int32_t width, int vertical, void *stream)
    wide = dict(table)
    wide[name] = (table[name][0], [ctypes.c_int64 if i == 1 else t for i, t in enumerate(table[name][1])])
    diffs = prototype_differences(H.PROTOTYPES, wide, N.STRUCTS)
    assert len(diffs) == 1 and diffs[0].startswith(name + ": argument 1 is int32_t")

    name = "pbr_cook_torrance_weighted_mse_stack_step"
    short = dict(table)
    short[name] = (table[name][0], table[name][1][:-1])
    diffs = prototype_differences(H.PROTOTYPES, short, N.STRUCTS)
    assert len(diffs) == 1 and diffs[0].startswith(name + ": 13 arguments, 12 bound")

    wrong = dict(table, pbr_render_desc_size=(ctypes.c_int, []), pbr_adam_check=(ctypes.c_int, [ctypes.c_void_p] + table["pbr_adam_check"][1][1:]))
    del wrong["pbr_abi_version"]
    assert [d.split(":")[0] for d in prototype_differences(H.PROTOTYPES, wrong, N.STRUCTS)] == ["pbr_abi_version", "pbr_adam_check", "pbr_render_desc_size"]

    class Swapped(ctypes.Structure):                                  # pbr_image_pack with `channels` and `bits` in each other's place
        _fields_ = [f for f in N.ImagePack._fields_[:5]] + [N.ImagePack._fields_[6], N.ImagePack._fields_[5]] + N.ImagePack._fields_[7:]
    assert ctypes.sizeof(Swapped) == ctypes.sizeof(N.ImagePack) and [f[0] for f in Swapped._fields_[5:7]] == ["bits", "channels"]
    diffs = layout_differences(layouts, dict(N.STRUCTS, pbr_image_pack=Swapped))
    assert sorted(d.split(":")[0] for d in diffs) == ["pbr_image_pack.bits", "pbr_image_pack.channels"]

    class Short(ctypes.Structure):                                    # pbr_map with a 4-byte stride: the size and the last offset move
        _fields_ = [("data", ctypes.c_void_p), ("batch_stride", ctypes.c_int32), ("channel_stride", ctypes.c_int64)]
    diffs = layout_differences(layouts, dict(N.STRUCTS, pbr_map=Short))
    assert [d.split(":")[0] for d in diffs] == ["pbr_map.batch_stride"] and ctypes.sizeof(Short) == 24

    mirror = native_integers()
    diffs, unmirrored = constant_differences(constants, dict(mirror, MAX_LIGHTS=mirror["MAX_LIGHTS"] + 1))
    assert diffs == ["PBR_MAX_LIGHTS: 16, binding 17"] and unmirrored == UNMIRRORED
    del mirror["ERR_UNSUPPORTED"]
    assert constant_differences(constants, mirror) == ([], UNMIRRORED | {"PBR_ERR_UNSUPPORTED"})
