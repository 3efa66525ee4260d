"""What lsmtree, sstable and memtable share in front of a device call: host
arrays to the device, zeroed device scratch, and the query batch of the get
paths.  torch is imported inside the functions, so importing the package still
needs no GPU; pack_keys is pure numpy."""
from __future__ import annotations

import numpy as np


def up(dev, a):
    """`a` as a contiguous uint8 view, copied and uploaded to `dev`."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def up_opt(dev, a):
    """up() for an optional array a kernel still takes a pointer for: None
    stays None, an empty array becomes 16 zero bytes."""
    if a is None:
        return None
    return up(dev, a) if np.asarray(a).size else u8(dev, 16)


def u8(dev, nbytes):
    """max(nbytes, 16) zero bytes on `dev`."""
    import torch
    return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def pack_keys(keys):
    """The query batch of nkv_lookup_dev, nkv_locate_dev and
    nkv_memtable_find_dev: (blob, koff, klen) with key i the klen[i] bytes at
    blob + koff[i].  klen is uint64, koff its exclusive sums, blob the keys
    (bytes(k) of each) end to end -- b"\\0" when every key is empty, so that
    the blob is never an empty upload."""
    keys = [bytes(k) for k in keys]
    klen = np.fromiter((len(k) for k in keys), dtype=np.uint64, count=len(keys))
    koff = np.zeros(len(keys), np.uint64)
    koff[1:] = np.cumsum(klen[:-1])
    return b"".join(keys) or b"\0", koff, klen
