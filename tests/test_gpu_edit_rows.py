"""spx_edit_warp_rows and spx_edit_unwarp_rows on the MI355X: every row compared with tests/edit_rows_ref.py for equality of bytes
(NEAREST, any element size) and of uint32 patterns (BLEND).

Two kinds of lists, as in tests/test_gpu_edit_lookup.py, whose planted streams and harness this file imports:
  planted   records the test writes itself -- no audio is processed, so every shape of list, track and launch can be set up
  real      the lists spx_batch_run_edits writes for the directed jobs, every row at hop = the plan's B, and the two identities
            that tie the row calls to spx_edit_lookup and spx_edit_replay_scaled, checked on the device.
Outputs and n_rows_out are pre-filled with canaries, with guard rows behind every region and guard columns between dim and ld: a
row that was not written, or a store outside the rows counted, is seen."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_lookup_ref as K  # noqa: E402
import edit_rows_ref as W  # noqa: E402
import test_gpu_edit_list as GE  # noqa: E402
import test_gpu_edit_lookup as GL  # noqa: E402  (SHAPES, synthetic, kinds, stream, Planted: imported, not copied)
import tsm_inputs as I  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0xA5                 # every byte of an output buffer before a call
COUNT_CANARY = -0x5a5a5a5a5a5a5a5a
GUARD_ROWS = 3
NEAREST, BLEND = 0, 1
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
_PLANS = {}


@pytest.fixture(scope="module")
def plan():
    from speedy_amd.batch import Plan
    p = Plan(16000, False)
    assert p.B == 160
    yield p
    p.close()


def limit(s):
    return K.limit_of(s["n_in"], 16000, s["nl"] != 0.0)


def key_cap(s):
    return s.get("key_cap", max(s["n_out"], 0) + 5)


def seen_ops(s):
    """The records the device may read: the first min(n_ops, cap)."""
    return s["ops"][:max(0, min(s["n_ops"], s["cap"]))].tolist()


def ref_plan(s, key, H, phi, n_rows, mode, unwarp):
    """The definition's plan for a planted stream, once per key (streams that share a key share records, counts and track length)."""
    k = (key, H, phi, n_rows, mode, unwarp)
    if key is None or k not in _PLANS:
        no = max(0, min(s["n_out"], key_cap(s)))
        p = W.unwarp_plan(seen_ops(s), no, limit(s), H, phi, n_rows) if unwarp else \
            W.warp_plan(seen_ops(s), no, limit(s), H, phi, n_rows, blend=mode == BLEND)
        if key is None:
            return p
        _PLANS[k] = p
    return _PLANS[k]


def make_track(n_rows, dim, eb, seed, special=False):
    """A track of random bytes (as float32: finite values; special: a NaN and an infinity in one row)."""
    rng = np.random.default_rng(seed)
    if eb == 4:
        y = (rng.standard_normal((max(n_rows, 1), dim)) * 300).astype(np.float32)
        if special and n_rows > 4:
            y[n_rows // 3, 0] = np.nan
            y[n_rows // 3, dim - 1] = np.inf if dim > 1 else np.nan
        return y[:n_rows].view(np.uint32)
    return rng.integers(1, 250, (n_rows, dim * eb), dtype=np.uint8).view(DTYPES[eb])


class Rows:
    """One call over planted streams: tracks laid out with strides, guard columns and guard rows; the output full of canaries."""

    def __init__(self, pl, streams, tracks, H, phi, dim, eb, unwarp=False, mode=NEAREST, pad=0, shift=0, out_caps=None, keys=None):
        import torch
        self.pl, self.streams, self.n = pl, streams, len(streams)
        self.H, self.phi, self.dim, self.eb, self.unwarp, self.mode = H, phi, dim, eb, unwarp, mode
        self.ld = dim + pad
        self.tracks, self.keys = tracks, keys or [None] * self.n
        for j, s in zip(pl.jobs, streams):
            j.out_cap = key_cap(s)
        from speedy_amd._lib import EditRowsTrack
        self.tr = (EditRowsTrack * self.n)()
        self.want_counts, self.caps = [], []
        in_off = out_off = 0
        for i, (s, y) in enumerate(zip(streams, tracks)):
            R = W.rows(limit(s) if unwarp else max(0, min(s["n_out"], key_cap(s))), H, phi)
            cap = R if out_caps is None or out_caps[i] is None else out_caps[i]
            t = self.tr[i]
            t.in_off, t.out_off, t.n_rows, t.out_cap = in_off, out_off, y.shape[0], cap
            self.caps.append(cap)
            self.want_counts.append(W.count(unwarp, s["n_out"], key_cap(s), s["n_ops"], s["cap"], limit(s), H, phi, cap))
            in_off += (y.shape[0] + 1) * self.ld
            out_off += (cap + GUARD_ROWS) * self.ld
        dt = DTYPES[eb]
        host = np.full(max(1, in_off), 0x77, np.uint8).repeat(eb).view(dt)         # (columns at or behind dim: never read)
        for t, y in zip(self.tr, tracks):
            if y.shape[0]:
                host[t.in_off:t.in_off + y.shape[0] * self.ld].reshape(-1, self.ld)[:, :dim] = y
        # `shift` elements in front of both buffers: base pointers that are aligned to the element only
        self.total_out = max(1, out_off)
        d_in = torch.zeros((host.size + shift) * eb + 16, dtype=torch.uint8).cuda()
        d_in[shift * eb:(shift + host.size) * eb] = torch.from_numpy(host.view(np.uint8)).cuda()
        self.d_in, self.in_ptr = d_in, d_in.data_ptr() + shift * eb
        self.d_out = torch.full(((self.total_out + shift) * eb + 16,), CANARY, dtype=torch.uint8).cuda()
        self.out_ptr = self.d_out.data_ptr() + shift * eb
        self.shift = shift
        self.d_count = torch.full((self.n + 2,), COUNT_CANARY, dtype=torch.int64).cuda()

    def call(self, **kw):
        import torch
        pl, L = self.pl, self.pl.plan.L
        a = dict(jobs=pl.jobs, ops=pl.d_ops.data_ptr(), caps=pl.caps_ptr(), nops=pl.d_nops.data_ptr(), nout=pl.d_nout.data_ptr(),
                 index=pl.d_index.data_ptr(), tracks=self.tr, hop=self.H, phase=self.phi, dim=self.dim, ld_in=self.ld, ld_out=self.ld,
                 eb=self.eb, mode=self.mode, y_in=self.in_ptr, y_out=self.out_ptr, count=self.d_count.data_ptr())
        a.update(kw)
        hs = torch.cuda.current_stream().cuda_stream
        if self.unwarp:
            rc = L.spx_edit_unwarp_rows(pl.plan.h, a["jobs"], self.n, a["ops"], a["caps"], a["nops"], a["nout"], a["index"], a["tracks"],
                                        a["hop"], a["phase"], a["dim"], a["ld_in"], a["ld_out"], a["eb"], a["y_in"], a["y_out"], a["count"], hs)
        else:
            rc = L.spx_edit_warp_rows(pl.plan.h, a["jobs"], self.n, a["ops"], a["caps"], a["nops"], a["nout"], a["tracks"], a["hop"],
                                      a["phase"], a["dim"], a["ld_in"], a["ld_out"], a["eb"], a["mode"], a["y_in"], a["y_out"], a["count"], hs)
        self.msg = L.spx_last_error().decode() if rc != 0 else ""
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return bool((self.d_out == CANARY).all()) and bool((self.d_count == COUNT_CANARY).all())

    def check(self, tag=""):
        """Counts, rows, guard columns, rows behind the count, guard rows, the bytes in front of and behind the buffer."""
        eb, dim, ld = self.eb, self.dim, self.ld
        cnt = self.d_count.cpu().numpy()
        assert cnt[:self.n].tolist() == self.want_counts and (cnt[self.n:] == COUNT_CANARY).all(), (tag, "counts", cnt[:8], self.want_counts[:8])
        raw = self.d_out.cpu().numpy()
        assert (raw[:self.shift * eb] == CANARY).all() and (raw[(self.shift + self.total_out) * eb:] == CANARY).all(), (tag, "outside the buffer")
        out = raw[self.shift * eb:(self.shift + self.total_out) * eb].view(DTYPES[eb])
        can = np.frombuffer(bytes([CANARY]) * eb, DTYPES[eb])[0]
        bad = []
        for i, (s, y) in enumerate(zip(self.streams, self.tracks)):
            t, c = self.tr[i], max(self.want_counts[i], 0)
            region = out[t.out_off:t.out_off + (self.caps[i] + GUARD_ROWS) * ld].reshape(-1, ld)
            if not (region[c:] == can).all() or not (region[:, dim:] == can).all():
                bad.append((i, "a store outside the rows counted"))
                continue
            if c:
                p = ref_plan(s, self.keys[i], self.H, self.phi, y.shape[0], self.mode, self.unwarp)
                want = W.render(p, y.view(np.float32) if self.mode == BLEND else y, dim).view(DTYPES[eb])
                assert want.shape[0] == c, (tag, i, want.shape, c)
                w = np.nonzero((region[:c, :dim] != want).any(axis=1))[0]
                if w.size:
                    bad.append((i, "row", int(w[0]), region[w[0], :dim][:6], want[w[0]][:6], p[w[0]]))
        assert bad == [], (tag, bad[:4])


def planted(plan, streams):
    pl = GL.Planted(plan, streams)
    pl.index()
    return pl


def all_three(pl, streams, H, phi, dim, eb, in_rows=None, out_rows=None, **kw):
    """Warp NEAREST, warp BLEND (float rows only) and unwarp over the same streams.  in_rows / out_rows: rows of the tracks on the
    input's / output's timeline (default: what covers [0, L) / [0, no))."""
    for unwarp, mode in ((False, NEAREST), (False, BLEND), (True, NEAREST)):
        if mode == BLEND and eb != 4:
            continue
        tracks = []
        for i, s in enumerate(streams):
            span = max(0, min(s["n_out"], key_cap(s))) if unwarp else limit(s)
            rows = (out_rows if unwarp else in_rows)
            n = -(-span // H) if rows is None else rows[i]
            tracks.append(make_track(n, dim, eb, 1000 + i, special=mode == BLEND))
        r = Rows(pl, streams, tracks, H, phi, dim, eb, unwarp=unwarp, mode=mode, **kw)
        assert r.call() == 0, r.msg
        r.check((H, phi, dim, eb, "unwarp" if unwarp else ("blend" if mode else "nearest"), kw.get("pad"), kw.get("shift")))
    return r


# ------------------------------------------------------------------ planted lists ------------------------------------------------------------------

@pytest.mark.parametrize("H,phi", [(1, 0), (2, 0), (2, 1), (160, 0), (160, 80), (160, 159), (320, 0), (320, 160), (320, 319)])
def test_streams_of_0_1_63_64_65_and_257_rows(plan, H, phi):
    """Below, at and above a wave, and more than one block of 256 rows: the same records, the output cut (warp) or the input ended
    (unwarp) where it leaves exactly that many rows."""
    name, long_up = GL.kinds()[0]
    at = long_up["n_out"]
    assert at > 257 * 320 + 320
    targets = [257, 0, 1, 63, 64, 65]
    ends = [0 if t == 0 else (t - 1) * H + phi + 1 for t in targets]
    assert [W.rows(e, H, phi) for e in ends] == targets and all(W.rows(e - 1, H, phi) == t - 1 for e, t in zip(ends, targets) if t)
    warp = [GL.stream(long_up["ops"], long_up["n_in"], e) for e in ends]
    pl = planted(plan, warp)
    for mode, eb, dim in ((NEAREST, 4, 1), (BLEND, 4, 5), (NEAREST, 2, 3)):
        r = Rows(pl, warp, [make_track(-(-300000 // H), dim, eb, 7, mode == BLEND)] * 6, H, phi, dim, eb, mode=mode)
        assert r.call() == 0, r.msg
        assert r.want_counts == targets
        r.check(("warp", H, phi, mode))
    back = [GL.stream(long_up["ops"], e, at) for e in ends]
    pl = planted(plan, back)
    r = Rows(pl, back, [make_track(-(-at // H), 3, 2, 8)] * 6, H, phi, 3, 2, unwarp=True)
    assert r.call() == 0, r.msg
    assert r.want_counts == targets
    r.check(("unwarp", H, phi))


def shape_streams():
    ops = np.asarray(GL.SHAPES, np.int32)
    total = int(ops[-1][0] + ops[-1][3])
    s = [GL.stream(ops, 4000, total), GL.stream(ops, 4000, 60), GL.stream(ops, 4000, 65), GL.stream(ops, 4000, 0),
         GL.stream(ops, 1999, total, nl=1.0), GL.stream(ops, 4000, total - 2), GL.stream(ops, 4000, total)]
    s[6]["key_cap"] = 100                                    # the key's out_cap cuts the output short of n_out
    return s, total


@pytest.mark.parametrize("H,phi", [(1, 0), (2, 1), (3, 1), (7, 6), (160, 80)])
def test_record_shapes_cuts_padding_and_short_tracks(plan, H, phi):
    """Records of one to three frames, slow-down-shaped cross-fades, a jump ahead: the whole list, a cut inside a record, a cut
    before a record, n_out = 0, L below the largest source (zero rows), the key's out_cap below n_out -- with tracks that cover
    everything, and with tracks two rows shorter than the sources reach (zero rows)."""
    streams, total = shape_streams()
    assert limit(streams[4]) == 1920 and max(a + n for _, a, b, n in GL.SHAPES) > 1920
    pl = planted(plan, streams)
    all_three(pl, streams, H, phi, 4, 4)
    short_in = [max(0, -(-2012 // H) - 2)] * 7
    short_out = [max(0, -(-max(0, min(s["n_out"], key_cap(s))) // H) - 2) for s in streams]
    all_three(pl, streams, H, phi, 3, 4, in_rows=short_in, out_rows=short_out)
    if H <= 7:                                               # (at hop 160 the 306 output frames are two rows)
        p = W.warp_plan(seen_ops(streams[0]), total, 4000, H, phi, short_in[0])
        assert any(r[0] < 0 for r in p), "no zero row from the short track"
        p = W.warp_plan(seen_ops(streams[4]), total, 1920, H, phi, -(-1920 // H))
        assert any(r[0] < 0 for r in p), "no zero row from a source at or behind L"


@pytest.mark.parametrize("eb", [1, 2, 4, 8])
def test_every_dim_stride_and_alignment(plan, eb):
    """dim 1, 3, 4, 5, 80 and 257 with ld = dim and ld = dim + 3, the base pointers aligned to 16 bytes and one element off: rows of
    one lane and of a whole wave, 16-byte moves, every narrower width, and the tail of single elements.  A speed-up list, a
    slow-down list (the unwarp needs the running maximum there) and the record shapes; float rows carry a NaN and an infinity."""
    ks = dict(GL.kinds())
    streams = [ks["down"], ks["up_short"], shape_streams()[0][0]]
    m = GL.ref(ks["down"])
    assert sum(1 for r, g in zip(m.R, m.G) if r < g) > 20
    pl = planted(plan, streams)
    keys = ["down", "up_short", "shapes"]
    for dim in (1, 3, 4, 5, 80, 257):
        for pad in (0, 3):
            for shift in (0, 1):
                all_three(pl, streams, 7, 3, dim, eb, pad=pad, shift=shift, keys=keys)


def test_lists_of_4096_and_4097_records(plan):
    """At and above the size a block stages in LDS: the same slow-down list cut at 4 096 and at 4 097 records."""
    ops, _ = GL.synthetic(11000, 9, True, periods=(2, 12))
    assert len(ops) > 4097
    streams = []
    for k in (4096, 4097):
        end = int(ops[k - 1][0] + ops[k - 1][3])
        streams.append(GL.stream(ops[:k], 11000, end - 3))
    pl = planted(plan, streams)
    all_three(pl, streams, 3, 1, 5, 4)
    all_three(pl, streams, 160, 80, 80, 2)


def test_a_capacity_one_row_short_and_dead_streams_between_good_ones(plan):
    """out_cap one row below the count: MINUS the count, every byte of the region still the canary.  Dead streams -- n_ops = -(count),
    n_ops above the capacity, n_ops = 0, n_out = -1, and for a warp n_out = 0 -- report 0, write nothing and harm no neighbour."""
    ks = dict(GL.kinds())
    a, b = ks["down"], ks["up_short"]
    dead = [GL.stream(a["ops"], a["n_in"], a["n_out"], n_ops=-len(a["ops"]), cap=len(a["ops"]) - 1),
            GL.stream(a["ops"], a["n_in"], a["n_out"], n_ops=len(a["ops"]) + 1),
            GL.stream(a["ops"], a["n_in"], a["n_out"], n_ops=0),
            GL.stream(b["ops"], b["n_in"], -1),
            GL.stream(b["ops"], b["n_in"], 0)]
    streams = [a, dead[0], b, dead[1], dead[2], a, dead[3], dead[4], b]
    pl = planted(plan, streams)
    H, phi = 7, 3
    for unwarp in (False, True):
        full = [W.rows(limit(s) if unwarp else s["n_out"], H, phi) for s in streams]
        caps = [None, None, full[2] - 1, None, None, None, None, None, None]
        tracks = [make_track(-(-(s["n_out"] if unwarp else s["n_in"]) // H) if s["n_out"] > 0 else 3, 5, 2, 50 + i) for i, s in enumerate(streams)]
        r = Rows(pl, streams, tracks, H, phi, 5, 2, unwarp=unwarp, out_caps=caps)
        assert r.call() == 0, r.msg
        want = [full[0], 0, -full[2], 0, 0, full[5], 0, full[7] if unwarp else 0, full[8]]
        assert r.want_counts == want and full[2] > 10, (r.want_counts, want)
        r.check("unwarp" if unwarp else "warp")


def test_2048_streams_of_a_few_rows(plan):
    """Five kinds of list round-robin, each with its own track: a stream served with a neighbour's table, records, index or track
    shows.  Hop 320: 3 to 90 rows a stream."""
    ks = GL.kinds()[1:]
    pick = [(i * 3 + i // 5) % 5 for i in range(2048)]
    streams = [ks[k][1] for k in pick]
    keys = [ks[k][0] for k in pick]
    pl = planted(plan, streams)
    base = {name: (make_track(-(-s["n_in"] // 320), 4, 4, 70 + k, True), make_track(-(-s["n_out"] // 320), 4, 4, 80 + k)) for k, (name, s) in enumerate(ks)}
    launches = C.c_int(0)
    for unwarp, mode in ((False, NEAREST), (False, BLEND), (True, NEAREST)):
        r = Rows(pl, streams, [base[k][1 if unwarp else 0] for k in keys], 320, 160, 4, 4, unwarp=unwarp, mode=mode, keys=keys)
        assert r.call() == 0, r.msg
        gx = plan.L.spx_debug_last_rows_grid(C.byref(launches))
        assert gx == 1 and launches.value == 1 and 0 < max(r.want_counts) <= 256
        r.check((unwarp, mode))


def test_65600_one_row_streams_take_a_second_launch(plan):
    """More streams than the grid's second dimension holds: 65 535 in the first launch, 65 in the second.  Every stream has its own
    record and one row of its own value."""
    n = 65600
    streams = [GL.stream([(0, 7 + i % 50, -1, 40 + i % 50)] if i % 3 else [(0, 7 + i % 50, 3 + i % 45, 40 + i % 50)], 700, 30 + i % 40) for i in range(n)]
    pl = planted(plan, streams)
    keys = [(i % 50, i % 45, i % 3 == 0, i % 40) for i in range(n)]
    launches = C.c_int(0)
    for unwarp in (False, True):
        tracks = [np.full((1, 2), 1 + i, np.uint32) for i in range(n)]
        if unwarp:
            H, phi = 1000, 20                     # one row, frame 20: forward(20) lies in [0, 30): row 0 of the track
        else:
            H, phi = 100, 10                      # one row, output frame 10; every source is below 100: row 0 of the track
        r = Rows(pl, streams, tracks, H, phi, 2, 4, unwarp=unwarp, keys=keys)
        assert r.call() == 0, r.msg
        gx = plan.L.spx_debug_last_rows_grid(C.byref(launches))
        assert gx == 1 and launches.value == 2 and r.want_counts == [1] * n
        cnt = r.d_count.cpu().numpy()
        assert (cnt[:n] == 1).all() and (cnt[n:] == COUNT_CANARY).all()
        out = r.d_out.cpu().numpy()[:r.total_out * 4].view(np.uint32).reshape(n, 1 + GUARD_ROWS, 2)
        assert np.array_equal(out[:, 0, 0], np.arange(1, n + 1, dtype=np.uint32)) and np.array_equal(out[:, 0, 1], out[:, 0, 0]), unwarp
        assert (out[:, 1:] == 0xA5A5A5A5).all()
        assert all(p[0][0] == 0 for p in (ref_plan(streams[i], None, H, phi, 1, NEAREST, unwarp) for i in (0, 1, 2, 49, 65535, 65599)))


def test_refusals_launch_nothing_and_a_good_call_works_right_after(plan):
    ks = dict(GL.kinds())
    streams = [ks["up_short"], ks["down"]]
    pl = planted(plan, streams)
    i64 = C.POINTER(C.c_int64)
    from speedy_amd._lib import EditRowsTrack
    bad_caps = [C.cast((C.c_int64 * 2)(5, -1), i64), C.cast((C.c_int64 * 2)(2 ** 31 - 1, 1), i64)]

    def tracks_with(**kw):
        tr = (EditRowsTrack * 2)()
        for t in tr:
            t.in_off, t.out_off, t.n_rows, t.out_cap = 0, 0, 10, 10
        for k, v in kw.items():
            setattr(tr[1], k, v)
        return tr

    for unwarp in (False, True):
        mk = lambda eb=4, mode=NEAREST: Rows(pl, streams, [make_track(-(-(s["n_out"] if unwarp else s["n_in"]) // 7), 5, eb, 3) for s in streams],  # noqa: E731
                                             7, 3, 5, eb, unwarp=unwarp, mode=mode)
        cases = [({"ops": None}, "NULL"), ({"caps": None}, "NULL"), ({"nops": None}, "NULL"), ({"nout": None}, "NULL"), ({"tracks": None}, "NULL"),
                 ({"y_in": None}, "NULL"), ({"y_out": None}, "NULL"), ({"count": None}, "NULL"),
                 ({"ops": pl.d_ops.data_ptr() + 8}, "aligned"), ({"caps": bad_caps[0]}, "negative capacity"), ({"caps": bad_caps[1]}, "2^31 - 1"),
                 ({"hop": 0}, "hop"), ({"hop": (1 << 20) + 1}, "hop"), ({"phase": -1}, "phase"), ({"phase": 7}, "phase"),
                 ({"dim": 0}, "dim"), ({"dim": 65537, "ld_in": 65537, "ld_out": 65537}, "dim"), ({"ld_in": 4}, "stride"), ({"ld_out": 4}, "stride"),
                 ({"eb": 3}, "elem_bytes"), ({"eb": 16}, "elem_bytes"), ({"eb": 0}, "elem_bytes"),
                 ({"tracks": tracks_with(in_off=-1)}, "negative"), ({"tracks": tracks_with(out_off=-1)}, "negative"),
                 ({"tracks": tracks_with(n_rows=-1)}, "negative"), ({"tracks": tracks_with(out_cap=-1)}, "negative")]
        if unwarp:
            cases.append(({"index": None}, "spx_edit_index"))
        else:
            cases += [({"mode": 2}, "mode"), ({"mode": -1}, "mode"), ({"mode": BLEND, "eb": 2}, "float32")]
        r = mk()
        cases += [({"y_in": r.in_ptr + 2}, "aligned"), ({"y_out": r.out_ptr + 1}, "aligned")]
        for kw, word in cases:
            rc = r.call(**kw)
            assert rc == -1 and word in r.msg and r.untouched(), (unwarp, list(kw), rc, r.msg)
        good = pl.jobs[1].speed
        pl.jobs[1].speed = float("nan")                       # a table spx_batch_run refuses
        rc = r.call()
        assert rc == -1 and "speed" in r.msg and r.untouched(), (rc, r.msg)
        pl.jobs[1].speed = good
        assert r.call() == 0, r.msg                          # ... and a good call right after, on the same buffers
        r.check("after the refusals")
        if not unwarp:
            r = mk(mode=BLEND)
            assert r.call(index=None) == 0, r.msg            # (a warp takes no index)
            r.check("blend after the refusals")


# ------------------------------------------------------------------ real lists ------------------------------------------------------------------

def _real(b, jobs, nonlinear, rate):
    """Every row of every stream at hop = B, phase B / 2, through Batch.warp_rows / unwarp_rows: int32 labels (dim 1), float32
    features (dim 3, blended), and the labels back -- against the definition over the list the GPU wrote.  Then the two identities."""
    B = rate // 100
    nout = GE._sync_np(b.d_nout)
    ms = [(b.edits(i).tolist(), int(nout[i]), K.limit_of(j[3].size // j[2], rate, nonlinear)) for i, j in enumerate(jobs)]
    labels = [np.arange(1, -(-L // B) + 1, dtype=np.int32).reshape(-1, 1) * 3 for _, _, L in ms]
    feats = [make_track(-(-L // B), 3, 4, 90 + i, True).view(np.float32) for i, (_, _, L) in enumerate(ms)]
    got_l, got_f = b.warp_rows(labels, B), b.warp_rows(feats, B, blend=True)
    back = b.unwarp_rows(got_l, B)
    blends = 0
    for i, (ops, no, L) in enumerate(ms):
        name = jobs[i][0]
        want = W.warp(ops, no, L, B, B // 2, labels[i], 1)
        assert got_l[i].dtype == np.int32 and got_l[i].shape == want.shape == (W.rows(no, B, B // 2), 1) and np.array_equal(got_l[i], want), name
        p = W.warp_plan(ops, no, L, B, B // 2, len(feats[i]), blend=True)
        blends += sum(1 for r in p if r[1] is not None)
        want = W.render(p, feats[i], 3)
        assert got_f[i].dtype == np.float32 and np.array_equal(got_f[i].view(np.uint32), want.view(np.uint32)), name
        want = W.unwarp(ops, no, L, B, B // 2, got_l[i], 1)
        count = W.count(True, no, no, len(ops), len(ops), L, B, B // 2, W.rows(L, B, B // 2))    # (0 for a job without a record: speed 2000)
        assert count in (0, len(want)) and back[i].shape == (count, 1) and np.array_equal(back[i], want[:count]), name
    assert blends > 20
    # identity 1: at hop 1 the NEAREST warp of the track (1, 2, .. L) is inverse(u) + 1, and 0 where inverse answers L
    ramp = [np.arange(1, L + 1, dtype=np.int64).reshape(-1, 1) for _, _, L in ms]
    got = b.warp_rows(ramp, 1)
    inv = b.locate_all([np.arange(max(no, 0)) for _, no, _ in ms], inverse=True)
    for i, (ops, no, L) in enumerate(ms):
        assert np.array_equal(got[i].ravel(), np.where(inv[i] >= L, 0, inv[i] + 1)), jobs[i][0]
    # identity 2: at hop 1, BLEND, dim = channels, a track of L frames is the float replay at p = q = 1
    masters = [make_track(L, 2, 4, 120 + i, True).view(np.float32) for i, (_, _, L) in enumerate(ms)]
    got = b.warp_rows(masters, 1, blend=True)
    rep = b.replay_scaled([y.reshape(-1) for y in masters], 2, 1)
    for i, (ops, no, L) in enumerate(ms):
        assert all(a != bb for _, a, bb, _ in ops if bb >= 0), jobs[i][0]
        assert np.array_equal(got[i].reshape(-1).view(np.uint32), rep[i].view(np.uint32)), jobs[i][0]


@pytest.mark.parametrize("rate", [16000, 22050])
def test_every_row_of_the_linear_jobs(rate):
    from speedy_amd.batch import Plan
    jobs = GE._linear_jobs(rate)
    assert len(jobs) > 15
    plan = Plan(rate, False)
    try:
        _real(GL._edits_batch(plan, jobs, [GE._linear_def(j) for j in jobs]), jobs, False, rate)
    finally:
        plan.close()


@pytest.mark.parametrize("rate", [16000, 22050])
def test_every_row_of_the_nonlinear_jobs(orc, rate):
    from speedy_amd.batch import Plan
    jobs = GE._nonlinear_jobs(rate)
    assert len(jobs) >= 3
    plan = Plan(rate, False)
    try:
        _real(GL._edits_batch(plan, jobs, [GE._nonlinear_def(orc, j, False) for j in jobs]), jobs, True, rate)
    finally:
        plan.close()


# ------------------------------------------------------------------ Python, and the C example ------------------------------------------------------------------

def test_python_round_trip_and_the_value_error():
    import torch
    from speedy_amd.batch import Batch, Plan
    by = {j[0]: j for j in I.linear_jobs()}
    job = by["speeds/16000Hz/1ch/9001/3.5"]
    e = GE._linear_def(job)
    plan = Plan(16000, False)
    try:
        plain = Batch(plan, [9001], 1, 3.5, 0.0)
        with pytest.raises(ValueError, match="edits=True"):
            plain.warp_rows([np.zeros((5, 1), np.int32)], 160)
        with pytest.raises(ValueError, match="edits=True"):
            plain.unwarp_rows([np.zeros((5, 1), np.int32)], 160)
        b = Batch(plan, [9001], 1, 3.5, 0.0, edits=True)
        b.upload([job[3]])
        b.run()
        assert b._index_built is False
        labels = np.arange(100, 100 + 57, dtype=np.int32)                                  # 1-D: dim 1; 57 rows cover 9001 frames
        out = b.warp_rows([labels], 160)[0]                                                # phase: hop // 2
        assert out.dtype == np.int32 and np.array_equal(out, W.warp(e.ops, e.out_n, e.limit, 160, 80, labels.reshape(-1, 1), 1))
        assert b._index_built is False
        back = b.unwarp_rows([torch.from_numpy(out)], 160)[0]                             # a torch tensor; builds the index
        assert b._index_built and np.array_equal(back, W.unwarp(e.ops, e.out_n, e.limit, 160, 80, out, 1))
        assert back.shape == (W.rows(9001, 160, 80), 1) and set(back.ravel().tolist()) <= set(labels.tolist()) | {0}
        f = make_track(57, 80, 4, 5).view(np.float32)
        assert np.array_equal(b.warp_rows([f], 160, phase=0, blend=True)[0].view(np.uint32),
                              W.warp(e.ops, e.out_n, e.limit, 160, 0, f, 80, blend=True).view(np.uint32))
        with pytest.raises(ValueError, match="float32"):
            b.warp_rows([labels], 160, blend=True)
        with pytest.raises(ValueError):
            b.warp_rows([labels], 160, phase=160)
    finally:
        plan.close()


def test_c_edit_rows_example(tmp_path):
    """tools/batch_edit_rows_example.c: a key, 100 Hz labels and 5-float features through the C ABI alone."""
    exe = os.path.join(ROOT, "speedy_amd", "lib", "batch_edit_rows_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "editrowsexample"])
    by = {j[0]: j for j in I.linear_jobs()}
    job = by["speeds/16000Hz/1ch/9001/3.5"]
    e = GE._linear_def(job)
    labels = (np.arange(57, dtype=np.int32) * 7 + 11).reshape(-1, 1)
    feats = make_track(57, 5, 4, 31).view(np.float32)
    job[3].tofile(tmp_path / "key.raw")
    labels.tofile(tmp_path / "labels.i32")
    feats.tofile(tmp_path / "feats.f32")
    r = subprocess.run([exe, str(tmp_path / "key.raw"), "16000", "3.5", "0", str(tmp_path / "labels.i32"), str(tmp_path / "feats.f32"), "5"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    wl = W.warp(e.ops, e.out_n, e.limit, 160, 80, labels, 1)
    wf = W.warp(e.ops, e.out_n, e.limit, 160, 80, feats, 5, blend=True)
    cap_rows = W.rows(plan_capacity(9001, 3.5), 160, 80)
    padded = np.zeros((cap_rows, 1), np.int32)
    padded[:len(wl)] = wl
    back = W.unwarp(e.ops, e.out_n, e.limit, 160, 80, padded, 1)
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert lines[0] == ["frames", str(e.out_n), "ops", str(len(e.ops))]
    assert lines[1] == ["labels", "rows", str(len(wl)), "sum", str(int(wl.sum()))]
    assert lines[2] == ["features", "rows", str(len(wf)), "bits", str(int(wf.view(np.uint32).astype(np.uint64).sum()))]
    same = int((back[:57].ravel() == labels[:len(back)].ravel()).sum())
    assert lines[3] == ["back", "rows", str(len(back)), "sum", str(int(back.sum())), "same", str(same)] and len(lines) == 4


def plan_capacity(n_in, speed):
    from speedy_amd.batch import Plan
    p = Plan(16000, False)
    try:
        return p.out_capacity(n_in, speed, 0.0)
    finally:
        p.close()
