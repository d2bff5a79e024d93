"""The input check that the episodes and the trials on the message-level
auction share (fleet_input_check, csrc/fleet_loop_dev.h), at the shapes where
it can go wrong: n = 64 (one 64-bit mask, all of it), 65 (one bit of the
second mask, one lane of the second task slot, n * n no multiple of the block)
and 128 (both masks whole). The other BAD_INPUT tests of the two loops fly
n = 13.

Six copies of a case fly side by side. Swarms 1 to 4 are broken in vehicle
n - 1's row -- the last iteration of a wave's row loop -- at a column >= 64
where n > 64 (the lane's second task): swarms 1 and 2 name a vehicle twice, so
that one value is missing, and over the parameters the missing values hit
every 32-bit word of the row's mask (n = 128: 5, 40, 70 and 127; n = 65: 64,
the only bit of the second 64-bit mask, and 31; n = 64: 63 and 0); swarm 3
holds n, the smallest value out of range, swarm 4 0xFFFF. Where the missing
value does not stand at such a column, the row is first permuted (two entries
swapped: still a permutation) so that it does. On the delay entries, at
n = 65, swarm 1 holds a 0 and swarm 3 max_lat + 1 in the last off-diagonal
entry of the latency matrix, swarm 2 a 0 and a 200 on the diagonal, which are
ignored.

The flagged swarms are ACL_FLEET_BAD_INPUT and untouched bit for bit, their
history rows stay 0; the others fly as the case does alone; after the repair
the next call flies all six."""
import functools

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_delay_episode_cases as DE
import fleet_delay_trial_cases as DT
import fleet_episode_cases as KE
import fleet_trial_cases as KT
import test_gpu_fleet_delay_episode as GDE
import test_gpu_fleet_delay_trial as GDT
import test_gpu_fleet_episode as GE
import test_gpu_fleet_trial as GT
from test_gpu_fleet_episode import _bits, _t, _u16

pytestmark = pytest.mark.gpu

B = 6
BAD_INPUT = 0x4  # ACL_FLEET_BAD_INPUT


@functools.lru_cache(maxsize=None)
def _episode_case(name):
    if name == "ring64":  # fleet_episode_cases.ring65's twin
        return KE.Case("ring64", C.clean_ring(64), steps=45, ticks_per_step=10, auction_every=45)
    return KE.case(name)


@functools.lru_cache(maxsize=None)
def _trial_case(name):
    if name == "ring64":  # fleet_trial_cases.ring65's twin
        sc = C.clean_ring(64)
        return KT.Case("ring64", [KT._ring_form(sc)], [0], sc.windows[0][1], 60, 10, tp=KT.QUICK,
                       ep=KT.DEFAULT_EVERY)
    return KT.case(name)


class _Episodes:
    """B copies of an episode case as one FleetEpisode; the bad input goes in
    after construction."""
    STATE = GE.STATE
    lead = 0

    def __init__(self, cs, copies, delay=False):
        self.obj = (GDE._episode if delay else GE._episode)([cs] * copies)

    def state(self):
        return GE._state(self.obj)

    def flags(self):
        return self.obj.status()["fleet"]["flags"].tolist()


class _Trials:
    """B swarms flying a trial case's one formation as one FleetTrial; the bad
    input goes in after the first step."""
    STATE = GT.STATE
    lead = 1

    def __init__(self, cs, copies, delay=False):
        extra = [((0,), cs)] * (copies - 1)
        self.obj = GDT._trial(GDT._lat_batch([cs], extra)) if delay else \
            GT._trial(GT._batch([cs], extra))

    def state(self):
        return GT._state(self.obj)

    def flags(self):
        return self.obj.fleet_status()["fleet"]["flags"].tolist()


def _flown(loop, cs, delay, steps):
    """The state of the case flown alone for `steps` steps."""
    alone = loop(cs, 1, delay)
    alone.obj.run(steps)
    return alone.state()


def _check(loop, cs, delay, write_bad, write_good, bad):
    """write_bad(obj) breaks the swarms `bad`, write_good(obj) repairs them."""
    import torch
    x = loop(cs, B, delay)
    x.obj.run(loop.lead)
    write_bad(x.obj)
    before = x.state()
    h = x.obj.run(2, history=True)
    after = x.state()
    good = [b for b in range(B) if b not in bad]
    assert x.flags() == [BAD_INPUT if b in bad else 0 for b in range(B)]
    for b in bad:
        for k in loop.STATE:
            if k not in ("fst", "_status"):
                np.testing.assert_array_equal(_bits(after[k][b]), _bits(before[k][b]),
                                              err_msg=f"swarm {b}: {k}")
        for k in h:
            assert not h[k].cpu().numpy()[:, b].any(), f"swarm {b}: history {k}"
    ref = _flown(loop, cs, delay, loop.lead + 2)
    for b in good:
        for k in loop.STATE:
            np.testing.assert_array_equal(_bits(after[k][b]), _bits(ref[k][0]),
                                          err_msg=f"swarm {b}: {k}")
    assert 0 in good and B - 1 in good
    write_good(x.obj)
    x.obj.run(1)
    torch.cuda.synchronize()
    assert x.flags() == [0] * B


def _twice(row, col, missing, dup):
    """The permutation `row` naming `dup` twice and `missing` not at all, the
    change standing at column col: `missing` is first swapped there."""
    row = row.copy()
    at = int(np.nonzero(row == missing)[0][0])
    row[at], row[col] = row[col], row[at]
    assert sorted(row.tolist()) == list(range(len(row))) and dup != missing
    row[col] = dup
    return row


# (case of the episodes, case of the trials) -> per loop the two duplicates
# (column, missing, named twice) and the column of the out-of-range entries
ROWS = {
    64: ("ring64", "ring64", {"episode": ((63, 63, 5), (32, 0, 40)),
                              "trial": ((63, 63, 31), (33, 0, 63))}, 63),
    65: ("ring65", "ring65", {"episode": ((64, 64, 0), (64, 31, 64)),
                              "trial": ((64, 64, 63), (64, 31, 64))}, 64),
    128: ("odd_last128", "near128", {"episode": ((127, 5, 127), (100, 70, 3)),
                                     "trial": ((64, 40, 64), (127, 127, 0))}, 96),
}


@pytest.mark.parametrize("n", sorted(ROWS))
@pytest.mark.parametrize("loop", [_Episodes, _Trials], ids=["episode", "trial"])
def test_bad_rows_in_the_last_row_and_the_second_task_slot(loop, n):
    ename, tname, dups, col = ROWS[n]
    episode = loop is _Episodes
    cs = _episode_case(ename) if episode else _trial_case(tname)
    assert cs.n == n
    good = {}

    def write_bad(obj):
        rows = obj.Pt.cpu().numpy().view(np.uint16).copy()
        good["rows"] = rows.copy()
        for b, (c, missing, dup) in zip((1, 2), dups["episode" if episode else "trial"]):
            assert c >= 64 or n <= 64
            rows[b, n - 1] = _twice(rows[b, n - 1], c, missing, dup)
        rows[3, n - 1, col] = n
        rows[4, n - 1, col] = 0xFFFF
        obj.Pt.copy_(_u16(rows))

    _check(loop, cs, False, write_bad, lambda obj: obj.Pt.copy_(_u16(good["rows"])),
           bad=(1, 2, 3, 4))


@pytest.mark.parametrize("loop", [_Episodes, _Trials], ids=["episode", "trial"])
def test_bad_latency_in_the_last_off_diagonal_entry_n65(loop):
    cs = DE.case("ring65_draw") if loop is _Episodes else DT.case("ring65_draw")
    n = 65
    assert cs.n == n and (n * n) % 256 != 0
    lat = np.stack([cs.lat] * B)
    bad = lat.copy()
    bad[1, n - 1, n - 2] = 0
    bad[3, n - 1, n - 2] = cs.max_lat + 1
    bad[2, 0, 0] = 0
    bad[2, n - 1, n - 1] = 200
    _check(loop, cs, True, lambda obj: obj.latency.copy_(_t(bad, np.uint8)),
           lambda obj: obj.latency.copy_(_t(lat, np.uint8)), bad=(1, 3))
