"""Event record layout shared by the host mirror, the synthetic generators and the tests.

Mirrors the in-memory layout of ``dvs_msgs::Event``
(reference: feature_tracker/src/dvs_msgs/Event.h:42-52): ``uint16 x; uint16 y;
ros::Time ts {uint32 sec; uint32 nsec}; uint8 polarity`` -> 16 bytes, AoS.
"""
import numpy as np

EVENT_DTYPE = np.dtype(
    {
        "names": ["x", "y", "sec", "nsec", "polarity"],
        "formats": ["<u2", "<u2", "<u4", "<u4", "u1"],
        "offsets": [0, 2, 4, 8, 12],
        "itemsize": 16,
    }
)


def make_events(x, y, t_us, polarity):
    """Pack arrays into an EVENT_DTYPE array. ``t_us`` are integer microseconds."""
    x = np.asarray(x)
    n = x.shape[0]
    ev = np.zeros(n, dtype=EVENT_DTYPE)
    t_us = np.asarray(t_us, dtype=np.int64)
    ev["x"] = x
    ev["y"] = np.asarray(y)
    ev["sec"] = (t_us // 1_000_000).astype(np.uint32)
    ev["nsec"] = ((t_us % 1_000_000) * 1000).astype(np.uint32)
    ev["polarity"] = np.asarray(polarity).astype(np.uint8)
    return ev


def event_times(ev):
    """ros::Time::toSec(): (double)sec + 1e-9*(double)nsec (two roundings, no FMA)."""
    return ev["sec"].astype(np.float64) + 1e-9 * ev["nsec"].astype(np.float64)


class EventFields:
    """Where the four fields of event i lie in caller-layout arrays (``esvio_fe_event_fields``): a base address and a
    byte stride per field, so separate arrays, aligned and packed structured records, slices and offset views are all
    described as they are — nothing is copied.  ``t``: uint32 (unsigned) or int64 ticks of ``t_unit_ns`` (1 or 1000)
    nanoseconds, ``t_offset`` ticks are added to every stamp; ``p``: 8 or 16 bits read as signed, polarity = (p > 0).
    The arrays are kept alive by the object (``.keep``)."""

    def __init__(self, x, y, t, p, t_unit_ns=1000, t_offset=0):
        x, y, t, p = (np.asarray(a) for a in (x, y, t, p))
        for name, a, sizes in (("x", x, (2,)), ("y", y, (2,)), ("t", t, (4, 8)), ("p", p, (1, 2))):
            if a.ndim != 1 or a.dtype.kind not in "iub" or a.dtype.itemsize not in sizes or a.dtype.byteorder == ">":
                raise ValueError("field %s: a 1-d little-endian integer array of %s bytes per element" % (name, " or ".join(map(str, sizes))))
        if t.dtype.itemsize == 4 and t.dtype.kind != "u":
            raise ValueError("32-bit stamps are unsigned (uint32)")
        if t.dtype.itemsize == 8 and t.dtype.kind != "i":
            raise ValueError("64-bit stamps are signed (int64)")
        if not (len(x) == len(y) == len(t) == len(p)):
            raise ValueError("fields differ in length")
        if int(t_unit_ns) not in (1, 1000):
            raise ValueError("t_unit_ns must be 1 or 1000")
        self.n = len(x)
        self.keep = (x, y, t, p)
        self.t_bits, self.p_bits = 8 * t.dtype.itemsize, 8 * p.dtype.itemsize
        self.t_unit_ns, self.t_offset = int(t_unit_ns), int(t_offset)
        # (a one-element view has whatever stride numpy made up: the element's width is the stride that is always valid)
        self.strides = tuple(int(a.strides[0]) if len(a) > 1 else a.dtype.itemsize for a in self.keep)
        if min(self.strides) < 0:
            raise ValueError("reversed views are not supported")
        self.ptrs = tuple(int(a.ctypes.data) if len(a) else 0 for a in self.keep)

    @classmethod
    def from_arrays(cls, x, y, t, p, t_unit_ns=1000, t_offset=0):
        """separate arrays x[], y[], t[], p[] (views keep their strides)"""
        return cls(x, y, t, p, t_unit_ns, t_offset)

    @classmethod
    def from_structured(cls, rec, x="x", y="y", t="t", p="p", t_unit_ns=1000, t_offset=0):
        """a numpy structured array (aligned or packed) and the names of its four fields"""
        rec = np.asarray(rec)
        return cls(rec[x], rec[y], rec[t], rec[p], t_unit_ns, t_offset)

    @classmethod
    def at_pointers(cls, ptrs, strides, n, t_bits, p_bits, t_unit_ns=1000, t_offset=0, keep=None):
        """fields at raw addresses (device memory, say): ptrs / strides = four ints each, in x, y, t, p order"""
        self = cls.__new__(cls)
        self.n, self.keep = int(n), keep
        self.ptrs, self.strides = tuple(int(a) for a in ptrs), tuple(int(a) for a in strides)
        self.t_bits, self.p_bits, self.t_unit_ns, self.t_offset = int(t_bits), int(p_bits), int(t_unit_ns), int(t_offset)
        return self

    def spans(self):
        """per field the (address, bytes) range it covers"""
        w = (2, 2, self.t_bits // 8, self.p_bits // 8)
        return [(self.ptrs[k], (self.n - 1) * self.strides[k] + w[k] if self.n else 0) for k in range(4)]
