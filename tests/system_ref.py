"""A small Python model of SystemSlot for the tests: SystemRuleManager.loadSystemConf / checkSystem
(SystemRuleManager.java:183-340) over a Constants.ENTRY_NODE built from a plain LeapArray (LeapArray.java:116-202,
ArrayMetric.java), and StatisticSlot's updates of that node (StatisticSlot.java:71-75, 88-91, 106-109, 139-141).

Written from the Java sources, one call of the reference per method, so that it shares no formulation with the device
code: every read calls currentWindow(t) and sums values(t) — the buckets with t - start <= interval.
"""
import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
LONG_MAX = (1 << 63) - 1
STAT_MAX_RT = 5000  # SentinelConfig.statisticMaxRt default
PASS, BLOCK, EXCEPTION, SUCCESS, RT, OCCUPIED = range(6)
QPS, THREAD, RT_TYPE, LOAD, CPU = range(5)  # SG_SYSTEM_*
LIMIT_NAMES = ["qps", "thread", "rt", "load", "cpu"]


class SystemConf:
    """SystemRuleManager's static fields after loadRules(rules); rules: (load, cpu, qps, avg_rt, max_thread)."""

    def __init__(self, rules=()):
        self.restore()
        if rules is not None and len(rules) >= 1:
            for r in rules:
                self.load_conf(*r)
        else:
            self.check = False

    def restore(self):
        self.check = False
        self.highest_load = self.highest_cpu = self.qps = DBL_MAX
        self.max_rt = self.max_thread = LONG_MAX
        self.load_set = self.cpu_set = self.rt_set = self.thread_set = self.qps_set = False

    def load_conf(self, load=-1.0, cpu=-1.0, qps=-1.0, avg_rt=-1, max_thread=-1):
        status = False
        if load >= 0:
            self.highest_load = min(self.highest_load, load)
            self.load_set = status = True
        if cpu >= 0:
            if cpu > 1:
                pass  # "Ignoring invalid SystemRule"
            else:
                self.highest_cpu = min(self.highest_cpu, cpu)
                self.cpu_set = status = True
        if avg_rt >= 0:
            self.max_rt = min(self.max_rt, avg_rt)
            self.rt_set = status = True
        if max_thread >= 0:
            self.max_thread = min(self.max_thread, max_thread)
            self.thread_set = status = True
        if qps >= 0:
            self.qps = min(self.qps, qps)
            self.qps_set = status = True
        self.check = status


class Leap:
    """LeapArray<MetricBucket>(sample_count, interval_ms)."""

    def __init__(self, sample_count, interval_ms):
        self.S, self.interval = sample_count, interval_ms
        self.wl = interval_ms // sample_count
        self.start = [None] * sample_count
        self.c = [[0] * 6 for _ in range(sample_count)]
        self.min_rt = [STAT_MAX_RT] * sample_count

    def current(self, t):
        i = (t // self.wl) % self.S
        ws = t - t % self.wl
        if self.start[i] is None or ws > self.start[i]:
            self.start[i] = ws
            self.c[i] = [0] * 6
            self.min_rt[i] = STAT_MAX_RT
        assert self.start[i] == ws, "time went backwards"
        return i

    def valid(self, t):
        return [i for i in range(self.S) if self.start[i] is not None and not t - self.start[i] > self.interval]

    def total(self, t, ev):
        self.current(t)
        return sum(self.c[i][ev] for i in self.valid(t))

    def max_success(self, t):
        self.current(t)
        return max([1] + [self.c[i][SUCCESS] for i in self.valid(t)])

    def min_rt_of(self, t):
        self.current(t)
        return max(1, min([STAT_MAX_RT] + [self.min_rt[i] for i in self.valid(t)]))

    def dump(self):
        """[S][8] in the layout of sg_local_read_state's second window."""
        out = np.zeros((self.S, 8), np.int64)
        for i in range(self.S):
            if self.start[i] is None:
                out[i, 0] = np.iinfo(np.int64).min
            else:
                out[i] = [self.start[i]] + self.c[i] + [self.min_rt[i]]
        return out


class EntryNode:
    """Constants.ENTRY_NODE: its second window and curThreadNum, and the slot that reads it."""

    def __init__(self, sample_count, interval_ms):
        self.w = Leap(sample_count, interval_ms)
        self.isec = interval_ms / 1000.0
        self.threads = 0

    # --- SystemRuleManager.checkSystem for an inbound entry: None, or the limit type
    def check(self, conf, t, count, load=-1.0, cpu=-1.0):
        if not conf.check:
            return None
        w = self.w
        if w.total(t, PASS) / self.isec + count > conf.qps:
            return QPS
        cur = self.threads
        if cur > conf.max_thread:
            return THREAD
        succ = w.total(t, SUCCESS)
        avg_rt = 0.0 if succ == 0 else w.total(t, RT) * 1.0 / succ
        if avg_rt > conf.max_rt:
            return RT_TYPE
        if conf.load_set and load > conf.highest_load:
            max_succ_qps = float(w.max_success(t)) * w.S / self.isec
            if cur > 1 and cur > max_succ_qps * float(w.min_rt_of(t)) / 1000:
                return LOAD
        if conf.cpu_set and cpu > conf.highest_cpu:
            return CPU
        return None

    # --- StatisticSlot
    def on_pass(self, t, count):
        self.threads += 1
        self.w.c[self.w.current(t)][PASS] += count

    def on_pass_wait(self):
        self.threads += 1

    def on_block(self, t, count):
        self.w.c[self.w.current(t)][BLOCK] += count

    def on_exit(self, t, create, count, error=False):
        i = self.w.current(t)
        rt = t - create
        self.w.c[i][SUCCESS] += count
        self.w.c[i][RT] += rt
        if rt < self.w.min_rt[i]:
            self.w.min_rt[i] = rt
        if error:
            self.w.c[i][EXCEPTION] += count
        self.threads -= 1


# ---------------------------------------------------------------- plain resources: the chain is StatisticSlot + SystemSlot

class PlainNode:
    """A StatisticNode of a resource without rules: second and minute windows, curThreadNum."""

    def __init__(self, sample_count, interval_ms):
        self.sec = Leap(sample_count, interval_ms)
        self.mnt = Leap(60, 60000)
        self.threads = 0

    def add(self, t, ev, n):
        self.sec.c[self.sec.current(t)][ev] += n
        self.mnt.c[self.mnt.current(t)][ev] += n

    def exit(self, t, create, count, error):
        rt = t - create
        for w in (self.sec, self.mnt):
            i = w.current(t)
            w.c[i][SUCCESS] += count
            w.c[i][RT] += rt
            w.min_rt[i] = min(w.min_rt[i], rt)
            if error:
                w.c[i][EXCEPTION] += count
        self.threads -= 1


class PlainChain:
    """Resources without flow, degrade, param or authority rules: an entry passes unless SystemSlot blocks it."""

    def __init__(self, n_res, inbound, sample_count=2, interval_ms=1000, flow_zero=()):
        self.S, self.interval, self.inbound = sample_count, interval_ms, list(inbound)
        # resources with one QPS flow rule of count 0 (DefaultController: (int) (passQps + count) > 0 blocks every
        # entry with count >= 1): arrivals that are no passes, for the bound of the clear proof
        self.flow_zero = set(flow_zero)
        self.entry = EntryNode(sample_count, interval_ms)
        self.nodes = {}  # (resource, None): the ClusterNode; (resource, origin id): its origin node
        self.conf = SystemConf()
        self.load = self.cpu = -1.0

    def node(self, res, origin=None):
        key = (res, origin)
        if key not in self.nodes:
            self.nodes[key] = PlainNode(self.S, self.interval)
        return self.nodes[key]

    def _touched(self, res, origin):
        out = [self.node(res)]
        if origin > 0:
            out.append(self.node(res, origin))
        return out

    def entry_event(self, t, res, count, origin):
        """(status, wait_ms) of SphU.entry."""
        inb = bool(self.inbound[res])
        nodes = self._touched(res, origin)  # ClusterBuilderSlot: created before any check
        kind = self.entry.check(self.conf, t, count, self.load, self.cpu) if inb else None
        if kind is not None:
            for n in nodes:
                n.add(t, BLOCK, count)
            self.entry.on_block(t, count)
            return 6, kind
        if res in self.flow_zero:
            assert count >= 1
            for n in nodes:
                n.add(t, BLOCK, count)
            if inb:
                self.entry.on_block(t, count)
            return 1, 0
        for n in nodes:
            n.threads += 1
            n.add(t, PASS, count)
        if inb:
            self.entry.on_pass(t, count)
        return 0, 0

    def exit_event(self, t, create, res, count, origin, error):
        for n in self._touched(res, origin):
            n.exit(t, create, count, error)
        if self.inbound[res]:
            self.entry.on_exit(t, create, count, error)
