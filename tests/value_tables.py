"""Adversarial values for the exact open-addressing value tables (tests/test_value_tables_gpu.py).

home() restates the tables' hash — the splitmix64 finaliser of v + 0x9E3779B97F4A7C15, masked to the sub-table
(sentinel_amd/csrc/pslot_dev.h:46-49 for param_slot, sentinel_amd/csrc/cparam_dev.h:30-33 for cp_slot / cp_find) —
only to choose inputs: values that all start their probe at one slot (the last one, so every chain wraps to slot 0).
No assertion depends on it; should the hash change, the values merely stop colliding and the tests get less sharp.
"""
import numpy as np

MARKER = 0xFFFFFFFFFFFFFFFF  # the tables' empty word; as a value it lives in the rule's side slot
M64 = (1 << 64) - 1


def home(v, mask):
    """First slot a value probes in a sub-table of mask + 1 slots."""
    h = (int(v) + 0x9E3779B97F4A7C15) & M64
    h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & M64
    h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & M64
    h ^= h >> 31
    return h & mask


def homed_values(rng, k, slot, mask, exclude=()):
    """k distinct ordinary values (never the marker, none of `exclude`) whose home in a mask + 1 slot table is `slot`."""
    out, seen = [], set(int(x) for x in exclude) | {MARKER}
    while len(out) < k:
        for v in rng.integers(0, 1 << 63, 64 * (mask + 1), dtype=np.uint64):
            v = (int(v) << 1 | int(v) & 1) & M64  # spread over the whole u64 range
            if v not in seen and home(v, mask) == slot:
                seen.add(v)
                out.append(v)
                if len(out) == k:
                    break
    return out


def random_values(rng, k, exclude=()):
    """k distinct ordinary values anywhere in the u64 range."""
    out, seen = [], set(int(x) for x in exclude) | {MARKER}
    while len(out) < k:
        v = (int(rng.integers(0, 1 << 63, dtype=np.uint64)) << 1 | int(rng.integers(0, 2))) & M64
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out
