"""np.savez_compressed with the members' time stamps pinned, so that a generator run twice writes the same bytes
(numpy stamps every member of the archive with the time of the run)."""
from __future__ import annotations

import io
import zipfile

import numpy as np


def savez_compressed_fixed(path, **arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    buf.seek(0)
    with zipfile.ZipFile(buf) as src, zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as dst:
        for name in src.namelist():
            info = zipfile.ZipInfo(name, date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            dst.writestr(info, src.read(name))
