"""TEST INFRASTRUCTURE -- reading and writing the torch fixtures under tests/golden/.

A fixture is stored as NAME.pt, or gzip-compressed as NAME.pt.gz when the plain file would exceed MAX_PLAIN_BYTES (no committed file
may be larger than 1 MiB).  Callers name the .pt path either way."""
import gzip
import io
import os

import torch

MAX_PLAIN_BYTES = 1 << 20


def load(path):
    if os.path.exists(path):
        return torch.load(path, weights_only=False)
    with gzip.open(path + ".gz", "rb") as f:
        return torch.load(io.BytesIO(f.read()), weights_only=False)


def save(obj, path):
    """-> the path written (path or path + ".gz"); the other form is removed so that load() cannot find a stale one."""
    buf = io.BytesIO()
    torch.save(obj, buf)
    data = buf.getvalue()
    if len(data) > MAX_PLAIN_BYTES:
        out, stale = path + ".gz", path
        data = gzip.compress(data, compresslevel=9, mtime=0)
    else:
        out, stale = path, path + ".gz"
    with open(out, "wb") as f:
        f.write(data)
    if os.path.exists(stale):
        os.unlink(stale)
    return out
