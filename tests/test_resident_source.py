"""The one-launch encode keeps its exchange (sweep, give-up count, fold of the missing slices,
reduce) once, as exchange_minmax in minmax_resident.hip -- except that the stack-order kernel
carries the same statements written out, because as a helper call they cost that kernel two
SGPRs and its f32 rows with R = 52 then spill.  This test keeps the two texts in step: a change
to the exchange that is made in one place only fails here, without a GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels", "minmax_resident.hip")


def statements(text):
    """Code lines without comments, blank lines and indentation."""
    out = []
    for line in text.splitlines():
        line = re.sub(r"//.*$", "", line).strip()
        if line:
            out.append(line)
    return out


def test_stack_kernel_exchange_is_the_helper_text():
    with open(SRC) as f:
        src = f.read()
    m = re.search(r"__device__ __forceinline__ MinMax exchange_minmax\([^)]*\)\s*\{\n(.*?)\n\}\n", src, re.S)
    assert m, "exchange_minmax not found"
    helper = statements(m.group(1))
    assert helper[0] == "constexpr int W = BLOCK / kWave;"
    helper = helper[1:]  # the kernel declares W itself, above the first mark
    assert helper[-1].startswith("return MinMax{") and helper[-1].endswith("};")
    helper[-1] = "const MinMax m{" + helper[-1][len("return MinMax{"):]

    marks = re.findall(r"// exchange_minmax: begin\n(.*?)// exchange_minmax: end\n", src, re.S)
    assert len(marks) == 1, "one written-out copy, in the stack-order kernel"
    stack = src.index("void minmax_resident_encode_kernel_stack(ResidentArgs a)")
    window = src.index("void minmax_resident_encode_kernel_window(ResidentArgs a)")
    assert stack < src.index("// exchange_minmax: begin") < window
    # the kernel passes its slice's chunk and LEAN = true (as the window kernel passes the helper)
    written = [s.replace("s.cl", "cl").replace("BLOCK, true>", "BLOCK, LEAN>") for s in statements(marks[0])]
    assert written == helper, "\n".join(["the stack kernel's exchange and exchange_minmax differ:"] +
                                        [f"  {a!r} != {b!r}" for a, b in zip(written, helper) if a != b])

    # every other kernel calls the helper
    assert len(re.findall(r"= exchange_minmax<T, BLOCK, (?:true|false)>\(a, s\.cl, tag, t, w, scratch\);", src)) == 2
