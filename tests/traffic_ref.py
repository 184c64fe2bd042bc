"""The traffic schedules' rule in plain Python integers: mix64, due, the lists, counts and totals.  The
only source of expected values of tests/test_traffic_ref.py and tests/test_gpu_traffic.py; E15 defines new behaviour, so nothing of
the reference is involved.  Written as the rule reads -- packet by packet -- not as the generator computes it."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MAX_PERIOD = 1 << 40
MAX_TIME = 1 << 62


def mix64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def valid(s):
    """s = (period_us, phase_us, jitter_us[, reserved])"""
    period, phase, jitter = (int(v) for v in s[:3])
    if len(s) > 3 and int(s[3]) != 0:
        return False
    if period == 0:
        return phase == 0 and jitter == 0
    return 1 <= period <= MAX_PERIOD and 0 <= phase < period and 0 <= jitter <= period


def jitter_of(s, seed, node, k):
    jitter = int(s[2])
    if jitter == 0:
        return 0
    h = mix64(mix64(mix64((int(seed) + GOLDEN) & M64) ^ (int(node) & 0xFFFFFFFF)) ^ (int(k) & M64))
    return (h * jitter) >> 64


def due(s, seed, node, k):
    return int(s[1]) + int(k) * int(s[0]) + jitter_of(s, seed, node, k)


def packets_in(s, seed, node, lo, hi):
    """the packet numbers of `node` with lo <= due < hi: a packet's due lies in [phase + k P, phase + k P + jitter], so only the k
    from (lo - phase - jitter) / P to (hi - 1 - phase) / P can be, and each of those is tested by its due itself"""
    period, phase, jitter = s[0], s[1], s[2]
    if period == 0 or hi <= lo or hi - 1 < phase:
        return []
    k0 = max(0, (lo - phase - jitter) // period)
    k1 = (hi - 1 - phase) // period
    return [k for k in range(k0, k1 + 1) if lo <= due(s, seed, node, k) < hi]


def may_send(s, lo, hi):
    """can the node have a packet in [lo, hi) at all: does the jitter interval of its first packet that ends at lo or later begin
    before hi (no packet is looked at)"""
    period, phase, jitter = s[0], s[1], s[2]
    if period == 0 or hi <= lo:
        return False
    k = max(0, -((phase + jitter - lo) // period))
    return phase + k * period < hi


def valid_windows(win_lo, win_hi):
    if len(win_lo) != len(win_hi) or len(win_lo) < 1:
        return False
    for b in range(len(win_lo)):
        if not 0 <= win_lo[b] <= win_hi[b] <= MAX_TIME:
            return False
        if b > 0 and win_hi[b - 1] > win_lo[b]:
            return False
    return True


def generate(table, seed, win_lo, win_hi, cap):
    """-> rows int32[n_ticks][cap] (ascending node indices, -1 behind them), count int32[n_ticks], totals, and the packets
    themselves as a set of (node, k)"""
    win_lo, win_hi = [int(v) for v in win_lo], [int(v) for v in win_hi]
    assert valid_windows(win_lo, win_hi) and cap >= 1
    n_ticks = len(win_lo)
    rows = np.full((n_ticks, cap), -1, dtype=np.int32)
    count = np.zeros(n_ticks, dtype=np.int32)
    packets, pairs, truncated = set(), 0, 0
    span_lo, span_hi = win_lo[0], win_hi[-1]
    active = [(i, tuple(int(v) for v in s)) for i, s in enumerate(table) if int(s[0]) > 0]
    # (a node that cannot have a packet in the whole span is skipped: the loop below would find nothing)
    active = [(i, s) for i, s in active if may_send(s, span_lo, span_hi)]
    for b in range(n_ticks):
        c = 0
        for i, s in active:
            ks = packets_in(s, seed, i, win_lo[b], win_hi[b])
            if not ks:
                continue
            packets.update((i, k) for k in ks)
            pairs += 1
            if c < cap:
                rows[b, c] = i
            c += 1
        count[b] = c
        truncated += max(0, c - cap)
    totals = {"packets": len(packets), "coalesced": len(packets) - pairs, "truncated": truncated}
    return rows, count, totals, packets


def lists_of(rows, count):
    """the rows as lists, clipped at cap"""
    return [rows[b, :min(int(count[b]), rows.shape[1])].tolist() for b in range(rows.shape[0])]


def table_rows(table):
    """(period, phase, jitter) rows -> an int64 [n][4] array, reserved 0"""
    a = np.zeros((len(table), 4), dtype=np.int64)
    for i, s in enumerate(table):
        a[i, :3] = [int(v) for v in s[:3]]
    return a
