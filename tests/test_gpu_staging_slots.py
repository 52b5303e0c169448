"""The pinned staging slots (SpxStage, speedy_amd/csrc/spx_engine.h) shared between call kinds on ONE stream with no host
synchronisation in between: a slot is re-acquired, grown and handed from one kind of call to the next while its previous reader
may still be in flight.

Seven calls on one 16 kHz plan and one HIP stream -- spx_batch_run (2 jobs), spx_batch_run_map (the same 2), spx_map_lookup,
spx_batch_run (a table that outgrows the slot's first allocation), spx_batch_run (2 jobs again), spx_batch_run_float (the large
table), spx_batch_pack_outputs -- then one synchronisation.  Every call's n_out and out, the map, the lookup results and the
packed output must equal, byte for byte, those of the same call made alone with a synchronisation after it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATE = 16000
N_IN = 1600                  # 0.1 s
SPEED, NONLINEAR = 2.5, 1.0
SMALL = 2
# The plan's slots take turns: the first plain call and the map call allocate one each, for a table of SMALL SpxStreamDev records
# (104 bytes each: spx_internal.h) and a tile order of at most two 4-byte entries per job (9 frames in tiles of 8 or more), by the
# growth rule 2 * bytes + 4096.  The large table must not fit that allocation.
STREAM_DEV_BYTES = 104
FIRST_CAP = 2 * (SMALL * STREAM_DEV_BYTES + SMALL * 2 * 4) + 4096
LARGE = 64
assert LARGE * STREAM_DEV_BYTES > FIRST_CAP
QUERIES = np.asarray([0, 160, 801, 1599, 1600], np.int64)
CANARY = 0x5a5a


def _sequence(alone):
    """The seven calls on a fresh plan, fresh buffers and a fresh stream.  alone: a synchronisation after every call; otherwise one
    at the end.  Returns {name: numpy array} of everything the calls wrote."""
    import torch
    from speedy_amd._lib import StreamJob
    from speedy_amd.batch import Plan
    from speedy_amd.synth import speech_like
    plan = Plan(RATE)
    L = plan.L
    dev = "cuda"
    try:
        cap = plan.out_capacity(N_IN, SPEED, NONLINEAR)
        region = (cap + 7) // 8 * 8
        jobs = (StreamJob * LARGE)()
        for i in range(LARGE):
            jobs[i] = StreamJob(i * N_IN, N_IN, i * region, cap, 1, SPEED, NONLINEAR, 0.0)
        x = np.concatenate([speech_like(N_IN, RATE, seed=40 + i) for i in range(LARGE)] + [np.zeros(64, np.int16)])
        d_in = torch.from_numpy(x).to(dev)
        d_inf = torch.from_numpy(x.astype(np.float32) / np.float32(32768)).to(dev)

        def ws_for(fn, n, *mid):
            b = fn(plan.h, jobs, *mid, n)
            assert b > 0, L.spx_last_error()
            return torch.zeros(b, dtype=torch.uint8, device=dev), b

        def outs(n, dtype=torch.int16, fill=CANARY):
            return (torch.full((n * region + 64,), fill, dtype=dtype, device=dev), torch.full((n,), -7, dtype=torch.int64, device=dev))

        rows = sum(L.spx_plan_map_rows(plan.h, N_IN, NONLINEAR) for _ in range(SMALL))
        d_map = torch.full((rows,), -12345, dtype=torch.int64, device=dev)
        d_qoff = torch.from_numpy(np.arange(SMALL + 1, dtype=np.int64) * QUERIES.size).to(dev)
        d_q = torch.from_numpy(np.tile(QUERIES, SMALL)).to(dev)
        d_r = torch.full((SMALL * QUERIES.size,), -1, dtype=torch.int64, device=dev)
        d_packed = torch.full((LARGE * region,), CANARY, dtype=torch.int16, device=dev)
        d_offsets = torch.full((LARGE + 1,), -1, dtype=torch.int64, device=dev)
        o1, o2, o4, o5 = outs(SMALL), outs(SMALL), outs(LARGE), outs(SMALL)
        o6 = outs(LARGE, torch.float32, 0.0)
        w1, w2, w4, w5 = (ws_for(L.spx_batch_workspace_bytes, n) for n in (SMALL, SMALL, LARGE, SMALL))
        w6 = ws_for(L.spx_batch_workspace_bytes_float, LARGE, None)
        stream = torch.cuda.Stream()
        hs = stream.cuda_stream
        torch.cuda.synchronize()   # the buffers above were filled on the default stream

        def done(rc):
            assert rc == 0, L.spx_last_error()
            if alone:
                stream.synchronize()

        def plain(n, o, w):
            return L.spx_batch_run(plan.h, jobs, n, d_in.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), w[0].data_ptr(), w[1], None, hs)

        done(plain(SMALL, o1, w1))
        done(L.spx_batch_run_map(plan.h, jobs, SMALL, d_in.data_ptr(), o2[0].data_ptr(), o2[1].data_ptr(), d_map.data_ptr(),
                                 w2[0].data_ptr(), w2[1], None, hs))
        done(L.spx_map_lookup(plan.h, jobs, SMALL, d_map.data_ptr(), d_qoff.data_ptr(), d_q.data_ptr(), d_r.data_ptr(), 0, hs))
        done(plain(LARGE, o4, w4))
        done(plain(SMALL, o5, w5))
        done(L.spx_batch_run_float(plan.h, jobs, None, LARGE, d_inf.data_ptr(), o6[0].data_ptr(), o6[1].data_ptr(), w6[0].data_ptr(),
                                   w6[1], None, hs))
        done(L.spx_batch_pack_outputs(jobs, LARGE, o4[0].data_ptr(), o4[1].data_ptr(), d_packed.data_ptr(), d_offsets.data_ptr(), hs))
        stream.synchronize()
        res = {"map": d_map, "lookup": d_r, "packed": d_packed, "offsets": d_offsets}
        for name, o in (("run2", o1), ("run_map", o2), ("run_large", o4), ("run2_again", o5), ("run_float", o6)):
            res[name + ".out"], res[name + ".n_out"] = o
        host = {k: v.cpu().numpy() for k, v in res.items()}
        return {k: a.view(np.uint32) if a.dtype == np.float32 else a for k, a in host.items()}   # (floats as bit patterns)
    finally:
        plan.close()


def test_calls_sharing_the_staging_slots_without_host_waits_equal_the_calls_made_alone():
    got = _sequence(alone=False)    # first: the plan's slots are new, the fourth call grows one of them
    want = _sequence(alone=True)
    for name in want:
        assert np.array_equal(got[name], want[name]), "%s differs from the same call made alone" % name
    # the calls did produce something: counts within the capacity, the map ends at the count, the lookup is monotonic
    for name in ("run2", "run_map", "run_large", "run2_again", "run_float"):
        assert (want[name + ".n_out"] > 0).all(), name
    assert np.array_equal(want["run_map.n_out"], want["run2.n_out"]) and np.array_equal(want["run_map.out"], want["run2.out"])
    assert np.array_equal(want["run_large.n_out"][:SMALL], want["run2.n_out"])
    # (an int16 value over 32768 is exact in float, and so is the nonlinear input scale's product: the float call sees the same samples)
    assert np.array_equal(want["run_float.n_out"], want["run_large.n_out"])
    rows = want["map"].reshape(SMALL, -1)
    assert np.array_equal(rows[:, -1], want["run_map.n_out"])
    look = want["lookup"].reshape(SMALL, -1)
    assert (np.diff(look, axis=1) >= 0).all() and np.array_equal(look[:, -1], rows[:, -1])
    assert want["offsets"][-1] == want["run_large.n_out"].sum() and (want["packed"][:want["offsets"][-1]] != CANARY).any()
