"""The sample-exact position lookup over an edit list as exact integers -- test infrastructure, CPU only.

include/speedy_hip.h "EDIT LIST" words the lookup (spx_edit_index, spx_edit_lookup); this file states it on Python integers.
Every output frame of a job is a copy of one input frame or a cross-fade of two (tests/edit_list_ref.py); its SOURCE is

  a record (out_at, a, b, n) covers output frames out_at + t, 0 <= t < n;  h = (n + 1) // 2, the number of t with 2 t < n
  copy (b < 0)     src = a + t
  cross-fade       src = a + t for t < h (the ramp going down still has the larger weight), else b + t (a tie in weight goes to the
                   ramp coming up)

With L as the replay has it (n_in for a linear job, (n_in // B) * B for a nonlinear one) and n_out the job's count:

  inverse(u)   u below 0 counts as 0; u >= n_out answers (L, -1); else k = the largest k with out_at(k) <= u and the answer is
               (min(src, L), k) -- a frame that plays flush padding answers L
  forward(p)   p clamped to [0, L]; the smallest output frame o < n_out with src(o) >= p, and its record; (n_out, -1) if there is none

src is not monotone in o (a slow-down plays input twice), so the searched form goes through R_k = the largest src inside record k
and its running maximum G_k = max(R_0 .. R_k): k = the first record with G_k >= p, then the first t with src >= p in closed form.
Lookup.forward / .inverse are that searched form; Lookup.brute_forward / .brute_inverse enumerate src over every output frame and
take the first -- tests/test_edit_lookup_definition.py holds the one to the other.  A stream whose n_ops or n_out is negative
answers (-1, -1) to everything.

SWITCHES make one mistake each:
  tie_to_a        2 t <= n keeps ramp a
  no_prefix_max   R searched where G belongs
  cut_ignored     no min with n_out in forward
  limit_n_in      L = n_in on a nonlinear job
"""
import bisect

SWITCHES = ("tie_to_a", "no_prefix_max", "cut_ignored", "limit_n_in")


def limit_of(n_in, rate, nonlinear, switch=None):
    """L: n_in for a linear job, (n_in // B) * B for a nonlinear one."""
    B = rate // 100
    return n_in // B * B if nonlinear and switch != "limit_n_in" else n_in


def half(n, switch=None):
    """How many t in [0, n) keep ramp a."""
    return min(n, n // 2 + 1) if switch == "tie_to_a" else (n + 1) // 2


def src(op, t, switch=None):
    """The source frame of output frame out_at + t of a record."""
    _, a, b, n = op
    return a + t if b < 0 or t < half(n, switch) else b + t


def record_max(op, switch=None):
    """R: the largest src inside a record."""
    _, a, b, n = op
    if b < 0:
        return a + n - 1
    h = half(n, switch)
    return max(a + h - 1, b + n - 1) if n > h else a + h - 1


def running_max(ops, switch=None):
    """G: what spx_edit_index writes, one value per record."""
    g, out = None, []
    for op in ops:
        r = record_max(op, switch)
        g = r if g is None or r > g else g
        out.append(g)
    return out


class Lookup:
    def __init__(self, ops, n_out, L, switch=None, n_ops=None):
        assert switch is None or switch in SWITCHES, switch
        self.ops = [tuple(int(v) for v in op) for op in ops]
        self.n_out, self.L, self.switch = int(n_out), int(L), switch
        self.dead = self.n_out < 0 or (n_ops is not None and n_ops < 0)
        self.out_at = [op[0] for op in self.ops]
        self.G = running_max(self.ops, switch)
        self.R = [record_max(op, switch) for op in self.ops]

    # ---- the searched form ----
    def inverse(self, u):
        if self.dead:
            return -1, -1
        u = max(int(u), 0)
        if u >= self.n_out or not self.ops:
            return self.L, -1
        k = max(bisect.bisect_right(self.out_at, u) - 1, 0)
        return min(src(self.ops[k], u - self.out_at[k], self.switch), self.L), k

    def forward(self, p):
        if self.dead:
            return -1, -1
        p = min(max(int(p), 0), self.L)
        # (the binary search for the first record at or above p; R does not rise where a slow-down plays input twice)
        k = bisect.bisect_left(self.R if self.switch == "no_prefix_max" else self.G, p)
        if k >= len(self.ops):
            return self.n_out, -1
        out_at, a, b, n = self.ops[k]
        t = max(0, p - a)
        if b >= 0:
            h = half(n, self.switch)
            if t >= h:
                t = max(h, p - b)
        o = out_at + t
        if self.switch != "cut_ignored":
            o = min(o, self.n_out)
        return (o, -1) if o == self.n_out else (o, k)

    # ---- the definition, enumerated ----
    def sources(self):
        """[(src, record)] of every output frame the list covers, the frames behind the cut included."""
        out = []
        for k, op in enumerate(self.ops):
            assert op[0] == len(out) and op[3] >= 1, "the enumeration takes a contiguous list"
            out += [(src(op, t, self.switch), k) for t in range(op[3])]
        return out

    def brute_inverse_all(self):
        """inverse(u) for u = 0 .. n_out."""
        if self.dead:
            return [(-1, -1)] * (self.n_out + 1 if self.n_out >= 0 else 1)
        s = self.sources()
        return [(min(s[u][0], self.L), s[u][1]) if u < len(s) else (self.L, -1) for u in range(self.n_out)] + [(self.L, -1)]

    def brute_forward_all(self):
        """forward(p) for p = 0 .. L: the first o < n_out with src(o) >= p, by one walk over the frames in order -- frame o answers
        every p above the sources heard so far and at or below its own."""
        if self.dead:
            return [(-1, -1)] * (self.L + 1)
        out = []
        for o, (v, k) in enumerate(self.sources()[:max(self.n_out, 0)]):
            while len(out) <= min(v, self.L):
                out.append((o, k))
        return out + [(self.n_out, -1)] * (self.L + 1 - len(out))
