"""The table set operations of tsx_hip_combine stated in plain Python over {k-mer: count} dicts -- the expectation of
tests/test_combine.py and tests/test_combine_cpu.py.  Nothing here calls the library.

a'(x) = a(x) if a_lower <= a(x) <= a_upper else 0 (a lower bound of 0 counts as 1), the same for b'.  Then
  intersect  x in OUT iff a' > 0 and b' > 0   count: min / max / sum (mod 2^64) / left = a' / right = b'
  union      x in OUT iff a' > 0 or b' > 0    both present: as intersect; one present: that one's count
  subtract   x in OUT iff a' > 0 and b' = 0   count a'
  diff       x in OUT iff a' > b'             count a' - b'
"""
M64 = (1 << 64) - 1
OPS = ("intersect", "union", "subtract", "diff")
MODES = ("min", "max", "sum", "left", "right")


def _ranged(c, rng):
    lo = max(1, int(rng[0]))
    hi = M64 if rng[1] is None else int(rng[1])
    return c if lo <= c <= hi else 0


def _both(mode, a, b):
    return {"min": min(a, b), "max": max(a, b), "sum": (a + b) & M64, "left": a, "right": b}[mode]


def combine_expect(A, B, op="intersect", mode="min", a_range=(1, None), b_range=(1, None)):
    """(OUT as {k-mer: count}, the tsx_hip_combine_stats as a dict)."""
    assert op in OPS and mode in MODES
    out = {}
    st = dict(a_in_range=0, b_in_range=0, both=0, a_sum_both=0, b_sum_both=0)
    for x in set(A) | set(B):
        a = _ranged(A.get(x, 0), a_range)
        b = _ranged(B.get(x, 0), b_range)
        st["a_in_range"] += a > 0
        st["b_in_range"] += b > 0
        if a and b:
            st["both"] += 1
            st["a_sum_both"] += a
            st["b_sum_both"] += b
        if op == "intersect":
            if a and b:
                out[x] = _both(mode, a, b)
        elif op == "union":
            if a and b:
                out[x] = _both(mode, a, b)
            elif a or b:
                out[x] = a or b
        elif op == "subtract":
            if a and not b:
                out[x] = a
        elif a > b:
            out[x] = a - b
    st["a_sum_both"] &= M64
    st["b_sum_both"] &= M64
    st["out_entries"] = len(out)
    st["out_count_sum"] = sum(out.values()) & M64
    return out, st


def jaccard(st):
    u = st["a_in_range"] + st["b_in_range"] - st["both"]
    return st["both"] / u if u else 0.0
