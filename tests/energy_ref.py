"""Expected values of the channel energy query from the oracle alone: a walk over frames x nodes
through orc_logdist_rssi / orc_det_pow10 / orc_det_log10, the Q80 sum kept in Python integers (to_fixed / from_fixed
restated from oracle/rm_oracle.c:337-370).  No engine code is involved."""
import ctypes as C
import math
import struct

import numpy as np

ED_TRANSMITTING, ED_BUSY = 1, 2
Q80_MAX = (1 << 127) - 1


def to_fixed(lin):
    if not lin > 0.0:
        return 0
    bits = struct.unpack("<Q", struct.pack("<d", lin))[0]
    ex = (bits >> 52) & 0x7FF
    if ex == 0x7FF:
        return Q80_MAX
    if ex == 0:
        return 0                                 # subnormal: below 2^-80 anyway
    man = (bits & 0x000FFFFFFFFFFFFF) | 0x0010000000000000
    shift = ex - 1075 + 80
    if shift >= 0:
        return Q80_MAX if shift > 74 else man << shift
    return 0 if -shift >= 64 else man >> (-shift)


def from_fixed(q):
    if q == 0:
        return 0.0
    top = q.bit_length() - 1
    if top <= 52:
        return math.ldexp(float(q), -80)
    drop = top - 52
    keep, rem, half = q >> drop, q & ((1 << drop) - 1), 1 << (drop - 1)
    if rem > half or (rem == half and (keep & 1)):
        keep += 1
    return math.ldexp(float(keep), drop - 80)    # keep may be 2^53: still exact


def channel_energy(O, mdl, nd, frames, t, nodes=None, channel=None, threshold=float("nan"), q80=False):
    """-> (energy float64[n], flags uint8[n], counting frames int32[n]) for `nodes` (default: all) at time t; `frames`: every
    frame handed to the medium so far (oracle PACKET_DTYPE; their recorded positions), nd: the node table as it is now.
    q80=True: a fourth value, the integer Q80 sum per node (Python integers)."""
    L = O.lib()
    ns = nd.as_struct()
    frames = np.ascontiguousarray(frames)
    nodes = np.arange(nd.n, dtype=np.int32) if nodes is None else np.asarray(nodes, dtype=np.int32)
    live = np.flatnonzero((frames["src"] >= 0) & (frames["start_us"] <= t) & (t < frames["start_us"] + frames["air_us"]))
    pk = [C.cast(frames[k:k + 1].ctypes.data, C.POINTER(O.Packet)) for k in live]
    fch, fsrc = frames["channel"][live].tolist(), frames["src"][live].tolist()
    sending = set(fsrc)
    noise = L.orc_det_pow10(mdl.ld_noise_dbm / 10.0)
    energy = np.empty(len(nodes))
    flags = np.zeros(len(nodes), dtype=np.uint8)
    counting = np.zeros(len(nodes), dtype=np.int32)
    sums = []
    for i, j in enumerate(nodes.tolist()):
        c = int(nd.channel[j]) if channel is None else channel
        acc = 0
        for p, pc, ps in zip(pk, fch, fsrc):
            if pc != c or ps == j:
                continue
            r = L.orc_logdist_rssi(C.byref(mdl), p, C.byref(ns), j)
            if r >= mdl.ld_ifloor_dbm:
                acc += to_fixed(L.orc_det_pow10(r / 10.0))
                counting[i] += 1
        sums.append(acc)
        energy[i] = 10.0 * L.orc_det_log10(from_fixed(acc) + noise)
        flags[i] = (ED_TRANSMITTING if j in sending else 0) | (ED_BUSY if energy[i] >= threshold else 0)
    return (energy, flags, counting, sums) if q80 else (energy, flags, counting)
