"""include/pbr_hip.h as the host tests read it: the text without its comments, and every prototype parsed into C type strings."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "include", "pbr_hip.h")
RAW = open(PATH).read()
TEXT = re.sub(r"/\*.*?\*/", "", RAW, flags=re.S)

_PROTOTYPE = re.compile(r"^[ \t]*(const char \*|int|size_t|void)\s*\b(pbr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", re.M)


def c_type(declaration):
    """'const pbr_render_desc *desc' -> 'pbr_render_desc *', 'void *const *data' -> 'void * *', 'int64_t' -> 'int64_t': the type of a
    parameter (its name, when it has one, dropped) without qualifiers, one blank between tokens."""
    tokens = [t for t in re.findall(r"\w+|\*", declaration) if t != "const"]
    if len(tokens) > 1 and tokens[-1] != "*":
        tokens.pop()                                     # the parameter's name
    return " ".join(tokens)


def prototypes(text=TEXT):
    """{name: (return type, [argument type, ...])} of every `<int | size_t | void | const char *> pbr_name(args);` of the header."""
    found = {}
    for ret, name, args in _PROTOTYPE.findall(text):
        assert name not in found, name
        args = [a.strip() for a in args.split(",")]
        found[name] = (c_type(ret + " _"), [] if args == ["void"] else [c_type(a) for a in args])
    return found


PROTOTYPES = prototypes()


def declared(name):
    """The parameter list of `name` as the header writes it (comments stripped), for assertions about one family's own arguments."""
    return re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, TEXT).group(1)
