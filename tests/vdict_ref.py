"""A Python model of the device value dictionary with its sweep (include/sentinel_gpu.h, sg_vdict_*): identity is
param_wire's canonical key (type tag, canonical payload), ids are positions that are never renumbered, a sweep frees
every id outside the live set and a later value takes the lowest free id before high + 1.

The fresh values of a batch are ranked by first appearance and rank r takes the r-th free id: the same as taking the
lowest free id one value at a time, which is what intern() does. The model also stands in for gateway_ref.Dictionary
(intern(bytes), ids, keys(), arena()), so a gateway_ref.Parser can number its strings through a swept dictionary."""
from sentinel_amd import abi
from sentinel_amd.param_wire import canonical_payload

STR = abi.PARAM_TYPE_STRING


def key_of(type_tag, payload):
    """The dictionary's key of a wire parameter."""
    return int(type_tag), canonical_payload(int(type_tag), bytes(payload))


class VDictModel:
    def __init__(self):
        self.ids = {}        # key → id, live values only
        self.key = {}        # id → key, live values only
        self.free = []       # ascending
        self.high = 0

    # ---- interning
    def intern_key(self, type_tag, payload):
        k = key_of(type_tag, payload)
        if k in self.ids:
            return self.ids[k]
        if self.free:
            i = self.free.pop(0)
        else:
            self.high += 1
            i = self.high
        self.ids[k], self.key[i] = i, k
        return i

    def intern_keys(self, keys):
        return [self.intern_key(t, p) for t, p in keys]

    def intern(self, s):     # gateway_ref.Dictionary: a STRING
        return self.intern_key(STR, s)

    def fresh(self, keys):
        """(distinct new values, their arena bytes) a batch of keys would add."""
        new = {key_of(t, p) for t, p in keys} - set(self.ids)
        return len(new), sum(len(p) for _, p in new if len(p) > 8)

    # ---- reading
    def size(self):
        return len(self.ids)

    def arena(self):
        return sum(len(p) for _, p in self.ids if len(p) > 8)

    def keys(self):
        """The live keys in id order (gateway_ref.Dictionary.keys when nothing was ever freed)."""
        return [self.key[i] for i in sorted(self.key)]

    def live_ids(self):
        return sorted(self.key)

    def dead_ids(self):
        return list(self.free)

    # ---- the sweep
    def sweep(self, live):
        """Frees every live id not in `live` (ids outside [1, high] and free ids in it are ignored, as table words
        are). Returns sg_vdict_sweep_stats."""
        live = set(int(x) for x in live)
        before = self.arena()
        gone = [i for i in self.key if i not in live]
        for i in gone:
            del self.ids[self.key.pop(i)]
        self.free = sorted(self.free + gone)
        assert len(self.key) + len(self.free) == self.high
        return {"live": len(self.key), "removed": len(gone), "free_ids": len(self.free), "high": self.high,
                "arena_before": before, "arena_after": self.arena()}
