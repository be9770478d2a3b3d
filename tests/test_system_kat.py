"""Known answers of the SystemSlot model in tests/system_ref.py (CPU): the SystemRuleManagerTest loads, hand-traced
answers of checkSystem for each limit type and their order, and the BBR boundary."""
from tests.system_ref import (BLOCK, CPU, DBL_MAX, LOAD, LONG_MAX, PASS, QPS, RT_TYPE, SUCCESS, THREAD, EntryNode, Leap,
                              PlainChain, SystemConf)

T0 = 1_700_000_000_000


def R(load=-1.0, cpu=-1.0, qps=-1.0, avg_rt=-1, max_thread=-1):
    return (load, cpu, qps, avg_rt, max_thread)


# ---- SystemRuleManagerTest

def test_load_invalid_rules():  # testLoadInvalidRules: every field negative
    c = SystemConf([R(load=-1, cpu=-1, qps=-4.0, avg_rt=-2, max_thread=-3)])
    assert not c.check
    assert (c.highest_load, c.highest_cpu, c.qps, c.max_rt, c.max_thread) == (DBL_MAX, DBL_MAX, DBL_MAX, LONG_MAX, LONG_MAX)


def test_load_and_get_rules():  # testLoadAndGetRules / testLoadDuplicateRules: the minimum of every field
    c = SystemConf([R(load=4.0, qps=500.0, avg_rt=300, max_thread=40), R(load=3.0, qps=800.0, avg_rt=100, max_thread=60)])
    assert c.check and c.load_set and not c.cpu_set
    assert (c.highest_load, c.qps, c.max_rt, c.max_thread) == (3.0, 500.0, 100, 40)
    assert c.highest_cpu == DBL_MAX


def test_cpu_above_one_is_ignored():
    c = SystemConf([R(cpu=1.5)])
    assert not c.check and not c.cpu_set and c.highest_cpu == DBL_MAX
    c = SystemConf([R(cpu=0.6), R(cpu=1.0), R(cpu=1.0001)])
    assert c.highest_cpu == 0.6 and c.cpu_set
    assert not c.check  # the last rule set nothing


def test_last_rule_decides_status():
    c = SystemConf([R(qps=10.0), R()])
    assert not c.check and c.qps == 10.0 and c.qps_set  # stored, but never checked
    c = SystemConf([R(), R(qps=10.0)])
    assert c.check


def test_empty_list_and_reload():
    assert not SystemConf([]).check
    assert not SystemConf(None).check
    c = SystemConf([R(qps=0.0)])  # 0 is a threshold
    assert c.check and c.qps == 0.0


# ---- LeapArray

def test_leap_window_sums_and_stale_buckets():
    w = Leap(2, 1000)
    w.c[w.current(T0 + 10)][PASS] += 3
    w.c[w.current(T0 + 510)][PASS] += 4
    assert w.total(T0 + 999, PASS) == 7
    assert w.total(T0 + 1000, PASS) == 4      # the first bucket's slot is reset by currentWindow
    assert w.start[0] == T0 + 1000 and w.c[0][PASS] == 0
    assert w.total(T0 + 1499, PASS) == 4
    assert w.total(T0 + 2600, PASS) == 0      # a gap longer than the interval
    assert w.start == [T0 + 1000, T0 + 2500]  # the stale bucket stays in its slot until touched


# ---- checkSystem, one limit type at a time

def node_with(passes=0, threads=0, exits=()):
    n = EntryNode(2, 1000)
    if passes:
        n.w.c[n.w.current(T0)][PASS] += passes
    n.threads = threads
    for rt, count in exits:
        n.threads += 1
        n.on_exit(T0, T0 - rt, count)
    return n


def test_checking_off_passes_everything():
    n = node_with(passes=10 ** 6, threads=10 ** 6)
    assert n.check(SystemConf([R(qps=1.0), R()]), T0, 1) is None


def test_qps():
    c = SystemConf([R(qps=10.0)])
    assert node_with(passes=9).check(c, T0 + 1, 1) is None      # 9 + 1 > 10 is false
    assert node_with(passes=10).check(c, T0 + 1, 1) == QPS
    assert node_with(passes=9).check(c, T0 + 1, 2) == QPS       # the entry's own count
    assert node_with(passes=10).check(c, T0 + 1000, 1) is None  # the bucket left the window
    n = EntryNode(2, 500)                                       # interval 0.5 s: pass / 0.5
    n.w.c[n.w.current(T0)][PASS] += 5
    assert n.check(c, T0, 1) == QPS and n.check(SystemConf([R(qps=11.0)]), T0, 1) is None


def test_thread():
    c = SystemConf([R(max_thread=3)])
    assert node_with(threads=3).check(c, T0, 1) is None  # equality passes
    assert node_with(threads=4).check(c, T0, 1) == THREAD


def test_rt():
    c = SystemConf([R(avg_rt=100)])
    assert node_with().check(c, T0, 1) is None                             # no success: avgRt 0
    assert node_with(exits=[(100, 1), (100, 1)]).check(c, T0, 1) is None   # 100.0 > 100 is false
    assert node_with(exits=[(100, 1), (101, 1)]).check(c, T0, 1) == RT_TYPE
    assert node_with(exits=[(300, 4)]).check(c, T0, 1) is None             # rt / success with batchCount 4: 75.0


def test_load_bbr_boundary():
    c = SystemConf([R(load=1.0)])
    # maxSuccessQps = max(1, 0) * 2 / 1.0 = 2, minRt = max(1, 5000) -> bound 10.0
    assert node_with(threads=50).check(c, T0, 1, load=1.0) is None   # load > highest is false: not armed
    assert node_with(threads=50).check(c, T0, 1, load=-1.0) is None  # status never set
    assert node_with(threads=10).check(c, T0, 1, load=1.5) is None   # 10 > 10.0 is false
    assert node_with(threads=11).check(c, T0, 1, load=1.5) == LOAD
    # one exit of rt 0: minRt = max(1, 0) = 1, maxSuccess 1 -> bound 0.002: every curThread > 1 blocks, 1 never does
    n = node_with(threads=0, exits=[(0, 1)])
    n.threads = 1
    assert n.check(c, T0, 1, load=9.0) is None
    n.threads = 2
    assert n.check(c, T0, 1, load=9.0) == LOAD
    # 500 successes in a bucket, minRt 4: 500 * 2 / 1 * 4 / 1000 = 4.0
    n = node_with(exits=[(4, 500)])
    n.threads = 4
    assert n.check(c, T0, 1, load=9.0) is None
    n.threads = 5
    assert n.check(c, T0, 1, load=9.0) == LOAD


def test_cpu():
    c = SystemConf([R(cpu=0.5)])
    assert node_with().check(c, T0, 1, cpu=0.5) is None
    assert node_with().check(c, T0, 1, cpu=0.51) == CPU
    assert node_with().check(c, T0, 1) is None


def test_order_of_the_checks():
    everything = SystemConf([R(load=1.0, cpu=0.1, qps=1.0, avg_rt=1, max_thread=1)])
    n = node_with(passes=5, threads=0, exits=[(50, 1)])
    n.threads = 5
    assert n.check(everything, T0, 1, load=2.0, cpu=0.9) == QPS  # QPS and thread both over: "qps"
    assert n.check(SystemConf([R(load=1.0, cpu=0.1, avg_rt=1, max_thread=1)]), T0, 1, load=2.0, cpu=0.9) == THREAD
    assert n.check(SystemConf([R(load=1.0, cpu=0.1, avg_rt=1)]), T0, 1, load=2.0, cpu=0.9) == RT_TYPE
    assert n.check(SystemConf([R(load=1.0, cpu=0.1)]), T0, 1, load=2.0, cpu=0.9) == LOAD
    assert n.check(SystemConf([R(cpu=0.1)]), T0, 1, load=2.0, cpu=0.9) == CPU


# ---- StatisticSlot's ENTRY_NODE updates through the plain chain

def test_plain_chain_counts_inbound_only():
    ch = PlainChain(2, [1, 0])
    ch.conf = SystemConf([R(qps=2.0)])
    assert ch.entry_event(T0, 0, 1, 0) == (0, 0)
    assert ch.entry_event(T0, 1, 5, 0) == (0, 0)       # outbound: neither checked nor counted
    assert ch.entry_event(T0 + 1, 0, 1, 1) == (0, 0)   # 1 + 1 > 2 is false
    assert ch.entry_event(T0 + 2, 0, 1, 1) == (6, QPS)
    e = ch.entry
    assert e.threads == 2 and e.w.total(T0 + 2, PASS) == 2 and e.w.total(T0 + 2, BLOCK) == 1
    assert ch.node(0).threads == 2 and ch.node(0, 1).threads == 1 and ch.node(1).threads == 1
    assert ch.node(0).sec.total(T0 + 2, BLOCK) == 1 and ch.node(0, 1).sec.total(T0 + 2, BLOCK) == 1
    ch.exit_event(T0 + 40, T0, 0, 1, 0, True)
    assert e.threads == 1 and e.w.total(T0 + 40, SUCCESS) == 1 and e.w.min_rt_of(T0 + 40) == 40
