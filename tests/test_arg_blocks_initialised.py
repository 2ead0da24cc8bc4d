"""CPU check of one rule of the native code: every object of a kernel-argument-block type is declared with an
initialiser (`T a{}`, `T a = ...`, a member `T m{}`), and no argument block is cleared with memset.  With `{}` every member without a
default initialiser is zero or nullptr, which is what the kernels read as "not used" for their optional members; `T a;` leaves those
members holding whatever was on the stack.  The matcher is first run on inline samples, so that a pattern that matches nothing fails."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "direct-visual-odometry_amd", "csrc")

# argument blocks whose names do not end in "Args"; every struct named *Args is one as well (arg_types)
EXTRA_TYPES = ("PersistLevel", "PersistMono", "MonoRef", "TileTerms", "SolveTerms")
NOT_A_TYPE = {"return", "sizeof", "else", "case", "delete", "new", "goto", "throw", "struct", "class", "typename"}


def strip_comments(src):
    """The source without comments; line numbers are kept."""
    src = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def arg_types(sources):
    found = {n for src in sources.values() for n in re.findall(r"\bstruct\s+(\w+Args)\s*\{", src)}
    return found | set(EXTRA_TYPES)


def _line(src, pos):
    return src.count("\n", 0, pos) + 1


def bare_declarations(sources, types):
    """(file, line, type, name) of every declaration of an argument block without an initialiser: `T a;`, `T a[N];`, `T a, b;`."""
    alt = "|".join(sorted(types))
    pat = re.compile(r"(?:^|[;{}])\s*(?:(?:static|const|constexpr|volatile|__shared__)\s+)*(?:dvo::)?(%s)\s+(\w+)\s*(?:\[[^\]]*\]\s*)*[;,]"
                     % alt, re.M)
    return [(f, _line(src, m.start(2)), m.group(1), m.group(2)) for f, src in sources.items() for m in pat.finditer(src)]


def _declared_type(sources, f, pos, name):
    """The type of the last declaration of `name` in file f before pos; else of any declaration of it (a struct member)."""
    pat = re.compile(r"(?:^|[;{}(,])\s*(?:(?:static|const|constexpr|volatile|struct)\s+)*([A-Za-z_][\w:]*)\s*[&*]*\s*\b%s\s*"
                     r"(?:\[[^\]]*\]\s*)*(?=[;,={)\[])" % re.escape(name), re.M)
    hits = [m.group(1) for m in pat.finditer(sources[f], 0, pos) if m.group(1) not in NOT_A_TYPE]
    if hits:
        return hits[-1].split("::")[-1]
    for g, src in sources.items():
        hits = [m.group(1) for m in pat.finditer(src) if m.group(1) not in NOT_A_TYPE]
        if hits:
            return hits[-1].split("::")[-1]
    return None


def memsets_of_arg_blocks(sources, types):
    """(file, line, target) of every memset whose target is declared with an argument-block type or whose size is sizeof(T)."""
    out = []
    for f, src in sources.items():
        for m in re.finditer(r"\bmemset\s*\(\s*&?\s*([\w.\->\[\]]+?)\s*,\s*[^,]+,\s*([^;]*);", src):
            target, size = m.group(1), m.group(2)
            name = re.split(r"\.|->", re.sub(r"\[[^\]]*\]", "", target))[-1]
            t = _declared_type(sources, f, m.start(), name)
            if t in types or any(re.search(r"\bsizeof\s*\(\s*(?:dvo::)?%s\s*\)" % x, size) for x in types):
                out.append((f, _line(src, m.start()), target))
    return out


def _check(sources):
    types = arg_types(sources)
    return types, bare_declarations(sources, types), memsets_of_arg_blocks(sources, types)


def test_matcher_on_samples():
    hdr = strip_comments("""
struct GnArgs { const float* p; int n = 1; };
struct SolveArgs{ int* q; };
struct PyramidArgs { const float* src[3]; };
struct PoseSeedArgs { int n = 0; };
struct FooArgs { int* p; int n = 1; };      // a new *Args type is covered without being listed
struct Holder {
    PersistMono tail;                       // bad: member without an initialiser
    PersistLevel lv[DVO_MAX_LEVELS];        // bad
    PersistMono ok_tail = {};
    PersistLevel ok_lv[DVO_MAX_LEVELS]{};
    const FooArgs* seed = nullptr;          // a pointer, not a block
};
void launch_foo(const FooArgs& a, hipStream_t s);
__global__ void k_foo(FooArgs a, GnArgs g, SolveArgs s) {}
""")
    src = strip_comments("""
void f(Holder& h, const FooArgs& in, float* buf)
{
    GnArgs a;                               // bad
    MonoRef r, q{};                         // bad (r)
    FooArgs x[2];                           // bad
    SolveArgs sa{};
    PyramidArgs pa = {};
    FooArgs y = in;
    PoseSeedArgs ps{}; /* PoseSeedArgs hidden; */
    memset(&sa, 0, sizeof sa);              // bad
    memset(&h.tail, 0, sizeof h.tail);      // bad: a member declared in the header
    memset(buf, 0, sizeof(FooArgs));        // bad: the size of a block
    float v[4]; memset(v, 0, sizeof v);
    memset(buf, 0, 16);
    if (1) { FooArgs z; }                   // bad
}
""")
    types, bare, sets = _check({"h.h": hdr, "s.cpp": src})
    assert types == {"GnArgs", "SolveArgs", "PyramidArgs", "PoseSeedArgs", "FooArgs"} | set(EXTRA_TYPES)
    assert sorted((f, t, n) for f, _, t, n in bare) == sorted([
        ("h.h", "PersistMono", "tail"), ("h.h", "PersistLevel", "lv"),
        ("s.cpp", "GnArgs", "a"), ("s.cpp", "MonoRef", "r"), ("s.cpp", "FooArgs", "x"), ("s.cpp", "FooArgs", "z")])
    assert sorted((f, t) for f, _, t in sets) == [("s.cpp", "buf"), ("s.cpp", "h.tail"), ("s.cpp", "sa")]


def test_every_arg_block_is_value_initialised():
    files = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")))
    assert len(files) >= 8
    sources = {os.path.basename(f): strip_comments(open(f).read()) for f in files}
    types, bare, sets = _check(sources)
    # the blocks of dvo_kernels.h and the one of dvo_kernels.hip must all be seen
    assert {"PyramidArgs", "GnArgs", "SolveArgs", "PersistArgs", "PropArgs", "UpdateArgs", "AgeTableArgs", "FusedArgs"} <= types
    assert not bare, "argument blocks declared without an initialiser (use T a{}): %s" % bare
    assert not sets, "memset of an argument block (use {} / x = {}): %s" % sets
