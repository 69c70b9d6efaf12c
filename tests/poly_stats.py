"""The `poly stats` lines that the C hosts print around a call on an operand edited behind the library's back (gpq_mpi_shim_poly_stats):
how far the call moved the resident-polynomial counters."""
import re


def edited_call_movement(lines):
    """(resident polynomials before the call, operands confirmed by it, operands found changed by it)"""
    seen = {}
    for x in lines:
        m = re.match(r"poly stats (before|after) the edited call: resident (\d+) confirmed (\d+) changed (\d+)$", x)
        if m:
            assert m.group(1) not in seen, "one edited call per run"
            seen[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    before, after = seen["before"], seen["after"]
    return before[0], after[1] - before[1], after[2] - before[2]
