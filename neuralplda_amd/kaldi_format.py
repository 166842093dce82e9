"""Native readers for the Kaldi objects the NPLDA initialisation consumes.

The reference shells out to Kaldi binaries (`copy-matrix`, `copy-vector`, `ivector-copy-plda`:
utils/models.py:442-448, utils/Kaldi2NumpyUtils/kaldiPlda2numpydict.py:17) and parses their text
output.  This module reads the same files directly — binary (`\\0B` + `FM `/`DM `/`FV `/`DV `
tokens, `\\x04`+int32 sizes, little-endian payload) or Kaldi text (`[ ... ]`) — so no Kaldi
installation is needed.  It is host-side file I/O only.

Feature matrices (`feats.scp` of a Kaldi data directory) are read too, including the compressed forms `CM` / `CM2` / `CM3`
that `make_mfcc.sh` writes by default: `read_matrix` decodes one on the host, `load_feature_scp` collects the raw bodies of
many into one buffer for the device decoder (neuralplda_amd/features.py, design/k13_feature_frontend.md).

16-bit PCM wave files (`wav.scp`) are read as well: `read_wav` for one file, `load_wav_scp` for many into one int16 buffer
for the MFCC kernel (neuralplda_amd/mfcc.py, design/k14_mfcc.md).

The objects themselves no longer have to come from Kaldi: neuralplda_amd/backend.py estimates `mean.vec`, `transform.mat`
and `plda` from x-vectors on the GPU, writes them with the writers below, and folds its arrays into a model through
`fold_arrays`, the array-level half of `fold_init` (design/k15_backend_estimation.md).
"""
import io
import os
import struct

import numpy as np

__all__ = ["read_vector", "read_matrix", "read_plda", "plda_psi_to_pq", "read_vector_ark", "read_vector_scp",
           "read_scp", "load_vector_ark", "load_vector_scp", "write_vector_ark", "fold_init",
           "write_matrix_binary", "write_vector_binary", "write_plda_binary", "read_feature_ark", "read_feature_scp",
           "load_feature_scp", "FeatureArchive", "FEAT_DESC", "FEAT_FORMATS", "KaldiFormatError", "read_wav",
           "load_wav_scp", "write_wav", "write_feature_ark", "fold_arrays"]


class KaldiFormatError(ValueError):
    pass


def _open(f):
    if isinstance(f, (bytes, bytearray)):
        return io.BytesIO(bytes(f)), True
    if hasattr(f, "read"):
        return f, False
    return open(f, "rb"), True


def _peek(fh, n):
    pos = fh.tell()
    b = fh.read(n)
    fh.seek(pos)
    return b


def _is_binary(fh):
    if _peek(fh, 2) == b"\0B":
        fh.read(2)
        return True
    return False


def _read_token(fh):
    """Whitespace-delimited token (binary mode tokens are followed by one space)."""
    tok = b""
    while True:
        c = fh.read(1)
        if not c:
            break
        if c in b" \t\r\n":
            if tok:
                break
            continue
        tok += c
    return tok.decode("ascii")


def _read_int32(fh):
    sz = fh.read(1)
    if sz != b"\x04":
        raise KaldiFormatError(f"expected int32 size marker \\x04, got {sz!r}")
    return struct.unpack("<i", fh.read(4))[0]


def _read_binary_vector_body(fh, tok):
    if tok not in ("FV", "DV"):
        raise KaldiFormatError(f"expected FV/DV vector token, got {tok!r}")
    dt = np.dtype("<f4") if tok == "FV" else np.dtype("<f8")
    n = _read_int32(fh)
    buf = fh.read(n * dt.itemsize)
    if len(buf) != n * dt.itemsize:
        raise KaldiFormatError("truncated vector payload")
    return np.frombuffer(buf, dtype=dt).astype(np.float64)


# Kaldi compressed-matrix.h, global header after the token: float min_value, float range, int32 num_rows, int32 num_cols
# (no \\x04 size markers).  CM: num_cols x four uint16 percentiles, then num_rows * num_cols bytes COLUMN-major; CM2: uint16
# row-major; CM3: uint8 row-major.
_CM_HEADER = struct.Struct("<ffii")


def _u16_to_float(min_value, rng, v):
    return min_value + rng * (1.0 / 65535.0) * v


def _decode_compressed(tok, min_value, rng, rows, cols, buf):
    """Body bytes of a CM / CM2 / CM3 matrix -> float64 (rows, cols)."""
    min_value, rng = float(min_value), float(rng)
    if tok == "CM2":
        return _u16_to_float(min_value, rng, np.frombuffer(buf, dtype="<u2").astype(np.float64)).reshape(rows, cols)
    if tok == "CM3":
        return (min_value + rng * (np.frombuffer(buf, dtype=np.uint8).astype(np.float64) / 255.0)).reshape(rows, cols)
    p = _u16_to_float(min_value, rng, np.frombuffer(buf, dtype="<u2", count=4 * cols).astype(np.float64)).reshape(cols, 4)
    b = np.frombuffer(buf, dtype=np.uint8, offset=8 * cols).astype(np.float64).reshape(cols, rows)
    p0, p25, p75, p100 = (p[:, i:i + 1] for i in range(4))
    out = np.where(b <= 64, p0 + (p25 - p0) * b / 64.0,
                   np.where(b <= 192, p25 + (p75 - p25) * (b - 64.0) / 128.0, p75 + (p100 - p75) * (b - 192.0) / 63.0))
    return np.ascontiguousarray(out.T)


def _compressed_body_bytes(tok, rows, cols):
    return {"CM": 8 * cols + rows * cols, "CM2": 2 * rows * cols, "CM3": rows * cols}[tok]


def _read_binary_matrix_body(fh, tok):
    if tok in ("CM", "CM2", "CM3"):
        hdr = fh.read(_CM_HEADER.size)
        if len(hdr) != _CM_HEADER.size:
            raise KaldiFormatError("truncated compressed-matrix header")
        min_value, rng, r, c = _CM_HEADER.unpack(hdr)
        if r < 0 or c < 0:
            raise KaldiFormatError(f"compressed matrix of {r} x {c}")
        n = _compressed_body_bytes(tok, r, c)
        buf = fh.read(n)
        if len(buf) != n:
            raise KaldiFormatError("truncated matrix payload")
        return _decode_compressed(tok, min_value, rng, r, c, buf)
    if tok not in ("FM", "DM"):
        raise KaldiFormatError(f"expected FM/DM/CM/CM2/CM3 matrix token, got {tok!r}")
    dt = np.dtype("<f4") if tok == "FM" else np.dtype("<f8")
    r = _read_int32(fh)
    c = _read_int32(fh)
    buf = fh.read(r * c * dt.itemsize)
    if len(buf) != r * c * dt.itemsize:
        raise KaldiFormatError("truncated matrix payload")
    return np.frombuffer(buf, dtype=dt).reshape(r, c).astype(np.float64)


def _read_text_vector_body(fh):
    """Text vector: ` [ v v v ]` (the opening bracket may already have been consumed)."""
    vals = []
    while True:
        tok = _read_token(fh)
        if tok == "":
            raise KaldiFormatError("unterminated text vector")
        if tok == "[":
            continue
        if tok == "]":
            break
        if tok.endswith("]"):
            vals.append(float(tok[:-1]))
            break
        vals.append(float(tok))
    return np.asarray(vals, dtype=np.float64)


def _read_text_matrix_body(fh):
    """Text matrix: ` [\\n r r r\\n r r r ]`."""
    text = b""
    while True:
        c = fh.read(1)
        if not c:
            raise KaldiFormatError("unterminated text matrix")
        text += c
        if c == b"]":
            break
    body = text.decode("ascii").replace("[", " ").replace("]", " ")
    rows = [ln.split() for ln in body.strip().split("\n") if ln.strip()]
    if not rows:
        return np.zeros((0, 0))
    return np.asarray(rows, dtype=np.float64)


def read_vector(f):
    """Kaldi Vector<float|double>, binary or text (e.g. Kaldi_Models/mean.vec) -> float64 (n,)."""
    fh, close = _open(f)
    try:
        if _is_binary(fh):
            return _read_binary_vector_body(fh, _read_token(fh))
        return _read_text_vector_body(fh)
    finally:
        if close:
            fh.close()


def read_matrix(f):
    """Kaldi Matrix<float|double> or CompressedMatrix, binary or text (e.g. Kaldi_Models/transform.mat) -> float64 (r, c)."""
    fh, close = _open(f)
    try:
        if _is_binary(fh):
            return _read_binary_matrix_body(fh, _read_token(fh))
        return _read_text_matrix_body(fh)
    finally:
        if close:
            fh.close()


def plda_psi_to_pq(psi):
    """Diagonal P/Q of the PLDA log-likelihood ratio from the between-class variances Psi
    (utils/Kaldi2NumpyUtils/kaldiPlda2numpydict.py:34-38)."""
    ac = np.asarray(psi, dtype=np.float64)
    tot = 1.0 + ac
    diagP = ac / (tot * (tot - ac * ac / tot))
    diagQ = (1.0 / tot) - 1.0 / (tot - ac * ac / tot)
    return diagP, diagQ


def read_plda(f):
    """Kaldi `Plda` object (ivector-compute-plda output), binary or text.  Returns the dict the
    reference builds (utils/Kaldi2NumpyUtils/kaldiPlda2numpydict.py:15-43): plda_mean,
    diagonalizing_transform, Psi_across_covar_diag, diagP, diagQ."""
    fh, close = _open(f)
    try:
        binary = _is_binary(fh)
        tok = _read_token(fh)
        if tok != "<Plda>":
            raise KaldiFormatError(f"expected <Plda>, got {tok!r}")
        if binary:
            mean = _read_binary_vector_body(fh, _read_token(fh))
            trans = _read_binary_matrix_body(fh, _read_token(fh))
            psi = _read_binary_vector_body(fh, _read_token(fh))
        else:
            mean = _read_text_vector_body(fh)
            trans = _read_text_matrix_body(fh)
            psi = _read_text_vector_body(fh)
        end = _read_token(fh)
        if end != "</Plda>":
            raise KaldiFormatError(f"expected </Plda>, got {end!r}")
    finally:
        if close:
            fh.close()
    diagP, diagQ = plda_psi_to_pq(psi)
    return {"plda_mean": mean, "diagonalizing_transform": trans, "Psi_across_covar_diag": psi,
            "diagP": diagP, "diagQ": diagQ}


def read_vector_ark(f):
    """Iterate (key, float32 vector) over a Kaldi vector archive (binary or text `key [ v ]` lines) —
    the x-vector ark format dataprep_*.py read through kaldi_io.read_vec_flt (dataprep_sre.py:152-167)."""
    fh, close = _open(f)
    try:
        while True:
            key = _read_token(fh)
            if key == "":
                return
            if _is_binary(fh):
                vec = _read_binary_vector_body(fh, _read_token(fh))
            else:
                vec = _read_text_vector_body(fh)
            yield key, vec.astype(np.float32)
    finally:
        if close:
            fh.close()


# ---- bulk x-vector readers: ark / scp -> ONE (N, D) float32 matrix ----------------------------
#
# dataprep_sre.py:152-167 builds the "mega dict" with one kaldi_io.read_vec_flt(rxfilename) call and one small numpy
# array per utterance, then pickles the dict (2-4 GB at VoxCeleb scale).  Here the archive is memory-mapped and the
# binary records are walked with a fixed-stride check: every `FV ` record of an x-vector ark has the same length, so
# after the keys are located all payloads are gathered with one strided numpy copy straight into a caller-provided
# (e.g. pinned) buffer — no per-utterance Python objects, no dict.

def read_scp(path):
    """Kaldi script file -> [(key, rxfilename)], rxfilename = 'file' or 'file:offset' (as dataprep_sre.py:158-160
    splits its lines: first blank separates key and rxfilename)."""
    out = []
    with open(path, "r") as fh:
        for ln in fh:
            ln = ln.rstrip("\n")
            if not ln.strip():
                continue
            key, _, rx = ln.partition(" ")
            out.append((key, rx.strip()))
    return out


def _split_rx(rx):
    """'path:offset' -> (path, offset) (offset None for a plain file; a ':' inside the path is kept)."""
    head, sep, tail = rx.rpartition(":")
    if sep and tail.isdigit():
        return head, int(tail)
    return rx, None


def _scp_file(f, scp_path):
    """An archive named by an scp entry: as written (Kaldi resolves against the working directory), else — for a relative
    name that is not there — next to the scp itself (an scp shipped in the same directory as its archive)."""
    if os.path.isabs(f) or os.path.exists(f):
        return f
    alt = os.path.join(os.path.dirname(os.path.abspath(scp_path)), f)
    return alt if os.path.exists(alt) else f


def _vec_at(buf, off):
    """float32 view of the (binary or text) vector whose object starts at byte `off` of `buf`."""
    if bytes(buf[off:off + 2]) == b"\0B":
        tok = bytes(buf[off + 2:off + 5])
        if tok not in (b"FV ", b"DV ") or buf[off + 5] != 4:
            raise KaldiFormatError(f"unexpected vector header {bytes(buf[off + 2:off + 10])!r}")
        n = int(np.frombuffer(buf, dtype="<i4", count=1, offset=off + 6)[0])
        dt = "<f4" if tok == b"FV " else "<f8"
        return np.frombuffer(buf, dtype=dt, count=n, offset=off + 10)
    end = bytes(buf[off:off + (1 << 16)]).find(b"]")
    return _read_text_vector_body(io.BytesIO(bytes(buf[off:off + end + 1])))


def read_vector_scp(path):
    """Iterate (key, float32 vector) over a Kaldi scp whose entries point at vectors ('ark:offset' or one-vector files):
    the exact replacement of `{key: kaldi_io.read_vec_flt(rx)}` at dataprep_sre.py:160."""
    maps = {}
    for key, rx in read_scp(path):
        f, off = _split_rx(rx)
        if f not in maps:
            maps[f] = np.memmap(_scp_file(f, path), dtype=np.uint8, mode="r")
        yield key, np.asarray(_vec_at(maps[f], off or 0), dtype=np.float32)


def _out_buffer(out, n, dim):
    if out is None:
        return np.empty((n, dim), dtype=np.float32)
    arr = out.numpy() if hasattr(out, "numpy") else out
    if arr.dtype != np.float32 or arr.ndim != 2 or arr.shape[0] < n or arr.shape[1] != dim:
        raise ValueError(f"out must be a float32 ({n}+, {dim}) buffer")
    return arr[:n]


def load_vector_ark(path, out=None):
    """Whole binary vector ark -> (keys, (N, D) float32 matrix).  `out`: optional pre-allocated float32 array or CPU
    torch tensor with >= N rows (pinned memory makes the following host-to-device copy asynchronous).  Falls back to
    the record-by-record reader for text archives or ragged records."""
    buf = np.memmap(path, dtype=np.uint8, mode="r")
    total = buf.shape[0]
    keys, offs = [], []
    pos = 0
    dim = None
    fast = True
    view = memoryview(buf)
    while pos < total:
        sp = bytes(view[pos:pos + 4096]).find(b" ")
        if sp < 0:
            break
        key = bytes(view[pos:pos + sp]).decode("ascii").strip()
        p = pos + sp + 1
        if bytes(view[p:p + 2]) != b"\0B" or bytes(view[p + 2:p + 5]) != b"FV " or view[p + 5] != 4:
            fast = False
            break
        n = int(np.frombuffer(buf, dtype="<i4", count=1, offset=p + 6)[0])
        if dim is None:
            dim = n
        elif n != dim:
            fast = False
            break
        keys.append(key)
        offs.append(p + 10)
        pos = p + 10 + 4 * n
    if not fast or dim is None:
        pairs = list(read_vector_ark(path))
        if not pairs:
            return [], np.zeros((0, 0), dtype=np.float32)
        mat = _out_buffer(out, len(pairs), pairs[0][1].shape[0])
        for i, (_, v) in enumerate(pairs):
            mat[i] = v
        return [k for k, _ in pairs], mat
    mat = _out_buffer(out, len(keys), dim)
    offs = np.asarray(offs, dtype=np.int64)
    idx = offs[:, None] + np.arange(4 * dim, dtype=np.int64)[None, :]
    # gather in slabs so the index matrix stays small (64k rows x 2 KB)
    step = 1 << 16
    m8 = mat.view(np.uint8).reshape(len(keys), 4 * dim)
    for lo in range(0, len(keys), step):
        m8[lo:lo + step] = buf[idx[lo:lo + step]]
    return keys, mat


def load_vector_scp(path, out=None):
    """Kaldi scp of x-vectors -> (keys, (N, D) float32 matrix), each archive memory-mapped once.  Entries of the form
    'ark:offset' that point at binary float vectors of one common length are gathered with one strided copy per
    archive; anything else goes through read_vector_scp."""
    entries = read_scp(path)
    if not entries:
        return [], np.zeros((0, 0), dtype=np.float32)
    by_file = {}
    for i, (_, rx) in enumerate(entries):
        f, off = _split_rx(rx)
        by_file.setdefault(f, []).append((i, off or 0))
    first_f, first_off = _split_rx(entries[0][1])
    probe = np.memmap(_scp_file(first_f, path), dtype=np.uint8, mode="r")
    dim = int(_vec_at(probe, first_off or 0).shape[0])
    mat = _out_buffer(out, len(entries), dim)
    m8 = mat.view(np.uint8).reshape(len(entries), 4 * dim)
    for f, lst in by_file.items():
        buf = np.memmap(_scp_file(f, path), dtype=np.uint8, mode="r")
        rows = np.asarray([i for i, _ in lst], dtype=np.int64)
        offs = np.asarray([o for _, o in lst], dtype=np.int64)
        hdr = buf[offs[:, None] + np.arange(10, dtype=np.int64)[None, :]]
        ok = (hdr[:, :6] == np.frombuffer(b"\0BFV \x04", dtype=np.uint8)).all() and \
            (hdr[:, 6:10].copy().view("<i4")[:, 0] == dim).all()
        if ok:
            step = 1 << 16
            for lo in range(0, len(rows), step):
                idx = offs[lo:lo + step, None] + 10 + np.arange(4 * dim, dtype=np.int64)[None, :]
                m8[rows[lo:lo + step]] = buf[idx]
        else:
            for i, o in lst:
                v = np.asarray(_vec_at(buf, o), dtype=np.float32)
                if v.shape[0] != dim:
                    raise KaldiFormatError(f"{entries[i][0]}: vector of length {v.shape[0]}, expected {dim}")
                mat[i] = v
    return [k for k, _ in entries], mat


def write_vector_ark(ark_path, keys, mat, scp_path=None):
    """Binary float-vector archive 'key \\0BFV \\x04<n>payload' per row (what copy-vector writes), optionally with the
    matching scp ('key ark_path:offset', offset = position of the \\0B marker).  One buffer, one write."""
    mat = np.ascontiguousarray(mat, dtype="<f4")
    n, dim = mat.shape
    if len(keys) != n:
        raise ValueError("one key per row")
    hdr = b"\0BFV \x04" + struct.pack("<i", dim)
    chunks, offsets, pos = [], [], 0
    for i, k in enumerate(keys):
        kb = k.encode("ascii") + b" "
        offsets.append(pos + len(kb))
        chunks.append(kb + hdr)
        chunks.append(mat[i].tobytes())
        pos += len(kb) + len(hdr) + 4 * dim
    with open(ark_path, "wb") as fh:
        fh.write(b"".join(chunks))
    if scp_path is not None:
        with open(scp_path, "w") as fh:
            fh.write("".join(f"{k} {ark_path}:{o}\n" for k, o in zip(keys, offsets)))
    return offsets


# ---- feature-matrix archives (feats.scp) ---------------------------------------------------------------------------
#
# The per-utterance loop of a feature reader (kaldi_io.read_mat per scp line, then NumPy per matrix) is what this avoids:
# the bodies are copied as they lie on disk into ONE buffer, and a descriptor per matrix tells the device decoder
# (csrc/nplda_feat.hip) where each is.  A CM matrix costs one byte per value on the way to the device, not four.

FEAT_FORMATS = {"FM": 0, "DM": 1, "CM": 2, "CM2": 3, "CM3": 4}  # include/nplda_hip.h NPLDA_FEAT_*
# nplda_feat_desc of include/nplda_hip.h (40 bytes); offsets in bytes from the start of the payload
FEAT_DESC = np.dtype([("format", "<i4"), ("rows", "<i4"), ("cols", "<i4"), ("min_value", "<f4"), ("range", "<f4"),
                      ("reserved", "<i4"), ("hdr_off", "<i8"), ("data_off", "<i8")])
_FEAT_ALIGN = 16  # every body starts on a 16-byte boundary of the payload (the decoder reads floats and doubles in place)


class FeatureArchive(tuple):
    """(keys, desc, payload) of load_feature_scp: keys in scp order, desc a FEAT_DESC array (one entry per key), payload
    ONE contiguous uint8 array holding the raw matrix bodies."""
    __slots__ = ()

    def __new__(cls, keys, desc, payload):
        return tuple.__new__(cls, (keys, desc, payload))

    keys = property(lambda self: self[0])
    desc = property(lambda self: self[1])
    payload = property(lambda self: self[2])

    def body(self, i):
        """The bytes of matrix i's data (for CM: without the per-column headers) as a view of the payload."""
        d = self.desc[i]
        esz = {0: 4, 1: 8, 2: 1, 3: 2, 4: 1}[int(d["format"])]
        return self.payload[int(d["data_off"]):int(d["data_off"]) + esz * int(d["rows"]) * int(d["cols"])]


def _matrix_header_at(buf, off, key):
    """(token, min_value, range, rows, cols, position of the body) of the binary matrix object at byte `off` of `buf`."""
    total = len(buf)
    head = bytes(buf[off:off + 32])
    if head[:2] != b"\0B":
        raise KaldiFormatError(f"{key}: not a binary Kaldi object at offset {off} (text-mode feature archives are not read)")
    sp = head.find(b" ", 2)
    tok = head[2:sp].decode("ascii", "replace") if sp > 0 else head[2:6].decode("ascii", "replace")
    pos = off + sp + 1
    if tok in ("FM", "DM"):
        if pos + 10 > total or buf[pos] != 4 or buf[pos + 5] != 4:
            raise KaldiFormatError(f"{key}: truncated or malformed {tok} header")
        r, c = struct.unpack("<i", bytes(buf[pos + 1:pos + 5]))[0], struct.unpack("<i", bytes(buf[pos + 6:pos + 10]))[0]
        return tok, 0.0, 0.0, r, c, pos + 10
    if tok in ("CM", "CM2", "CM3"):
        if pos + _CM_HEADER.size > total:
            raise KaldiFormatError(f"{key}: truncated {tok} header")
        mn, rg, r, c = _CM_HEADER.unpack(bytes(buf[pos:pos + _CM_HEADER.size]))
        return tok, mn, rg, r, c, pos + _CM_HEADER.size
    raise KaldiFormatError(f"{key}: unknown matrix token {tok!r} (expected FM, DM, CM, CM2 or CM3)")


def _body_bytes(tok, r, c):
    if tok in ("FM", "DM"):
        return r * c * (4 if tok == "FM" else 8)
    return _compressed_body_bytes(tok, r, c)


def read_feature_ark(f):
    """Iterate (key, float32 (T, D) matrix) over a binary Kaldi matrix archive whose entries are FM, DM, CM, CM2 or CM3,
    freely mixed (decoded on the host: a convenience; the bulk path is load_feature_scp + features.prepare_features)."""
    fh, close = _open(f)
    try:
        while True:
            key = _read_token(fh)
            if key == "":
                return
            if not _is_binary(fh):
                raise KaldiFormatError(f"{key}: text-mode feature archives are not read")
            try:
                mat = _read_binary_matrix_body(fh, _read_token(fh))
            except KaldiFormatError as e:
                raise KaldiFormatError(f"{key}: {e}") from None
            yield key, mat.astype(np.float32)
    finally:
        if close:
            fh.close()


def read_feature_scp(path):
    """Iterate (key, float32 (T, D) matrix) over a Kaldi scp of feature matrices ('ark:offset' or one-matrix files)."""
    maps = {}
    for key, rx in read_scp(path):
        f, off = _split_rx(rx)
        if f not in maps:
            maps[f] = np.memmap(_scp_file(f, path), dtype=np.uint8, mode="r")
        buf = maps[f]
        tok, mn, rg, r, c, pos = _matrix_header_at(buf, off or 0, key)
        n = _body_bytes(tok, r, c)
        if r < 0 or c < 0 or pos + n > len(buf):
            raise KaldiFormatError(f"{key}: truncated matrix payload ({tok} {r} x {c})")
        body = bytes(buf[pos:pos + n])
        if tok in ("FM", "DM"):
            mat = np.frombuffer(body, dtype="<f4" if tok == "FM" else "<f8").reshape(r, c)
        else:
            mat = _decode_compressed(tok, mn, rg, r, c, body)
        yield key, mat.astype(np.float32)


def load_feature_scp(path, entries=None, cols=None):
    """Kaldi scp of feature matrices -> FeatureArchive(keys, desc, payload) WITHOUT decoding: each archive is memory-mapped
    once and every entry's body (for CM: per-column headers, then data) is copied as it is into one uint8 buffer, each on a
    16-byte boundary.  `entries`: a slice of read_scp(path) to load instead of the whole file (bounded pieces of a large
    scp).  `cols`: if given, a matrix with another number of columns is an error naming the key."""
    if entries is None:
        entries = read_scp(path)
    n = len(entries)
    desc = np.zeros(n, dtype=FEAT_DESC)
    maps, src = {}, []
    total = 0
    for i, (key, rx) in enumerate(entries):
        f, off = _split_rx(rx)
        if f not in maps:
            maps[f] = np.memmap(_scp_file(f, path), dtype=np.uint8, mode="r")
        buf = maps[f]
        tok, mn, rg, r, c, pos = _matrix_header_at(buf, off or 0, key)
        nb = _body_bytes(tok, r, c)
        if r < 0 or c < 0 or pos + nb > len(buf):
            raise KaldiFormatError(f"{key}: truncated matrix payload ({tok} {r} x {c} needs {nb} bytes at {pos}, the archive "
                                   f"has {len(buf)})")
        if cols is not None and c != cols:
            raise KaldiFormatError(f"{key}: matrix of {c} columns, expected {cols}")
        hdr = 8 * c if tok == "CM" else 0
        desc[i] = (FEAT_FORMATS[tok], r, c, mn, rg, 0, total, total + hdr)
        src.append((buf, pos, nb, total))
        total += (nb + _FEAT_ALIGN - 1) // _FEAT_ALIGN * _FEAT_ALIGN
    payload = np.zeros(total, dtype=np.uint8)
    for buf, pos, nb, at in src:
        payload[at:at + nb] = buf[pos:pos + nb]
    return FeatureArchive([k for k, _ in entries], desc, payload)


# ---- 16-bit PCM audio (wav.scp) ----------------------------------------------------------------------------------------
#
# The audio counterpart of load_feature_scp: every file is memory-mapped, its RIFF chunks are walked, and the chosen
# channel's int16 samples are copied once into ONE buffer (no float copy on the host: the MFCC kernel reads int16).

_PCM_SUBFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")  # KSDATAFORMAT_SUBTYPE_PCM after its two-byte tag


def _wav_layout(buf, off, what):
    """(sample_rate, channels, byte position of the samples, sample frames) of the RIFF/WAVE object at byte `off` of `buf`:
    format tag 1, or 0xFFFE (extensible) with the PCM sub-format; 16 bits per sample."""
    total = len(buf)
    if off + 12 > total or bytes(buf[off:off + 4]) != b"RIFF" or bytes(buf[off + 8:off + 12]) != b"WAVE":
        raise KaldiFormatError(f"{what}: not a RIFF/WAVE file")
    pos, fmt = off + 12, None
    while pos + 8 <= total:
        cid = bytes(buf[pos:pos + 4])
        size = struct.unpack("<I", bytes(buf[pos + 4:pos + 8]))[0]
        body = pos + 8
        if cid == b"fmt ":
            if size < 16 or body + size > total:
                raise KaldiFormatError(f"{what}: truncated or malformed fmt chunk")
            tag, ch, rate, _, _, bits = struct.unpack("<HHIIHH", bytes(buf[body:body + 16]))
            if tag == 0xFFFE:
                if size < 40:
                    raise KaldiFormatError(f"{what}: extensible fmt chunk of {size} bytes")
                sub = bytes(buf[body + 24:body + 40])
                if sub[2:] != _PCM_SUBFORMAT_TAIL:
                    raise KaldiFormatError(f"{what}: extensible wave format whose sub-format is not PCM")
                tag = struct.unpack("<H", sub[:2])[0]
            if tag != 1:
                raise KaldiFormatError(f"{what}: wave format tag {tag}, only PCM (1) is read")
            if bits != 16:
                raise KaldiFormatError(f"{what}: {bits} bits per sample, only 16-bit PCM is read")
            if ch < 1:
                raise KaldiFormatError(f"{what}: {ch} channels")
            fmt = (rate, ch)
        elif cid == b"data":
            if fmt is None:
                raise KaldiFormatError(f"{what}: data chunk before the fmt chunk")
            if size == 0 or size == 0xFFFFFFFF:  # a streamed header: to the end of the file
                size = total - body
            elif body + size > total:
                raise KaldiFormatError(f"{what}: truncated data chunk ({size} bytes announced, {total - body} in the file)")
            return fmt[0], fmt[1], body, size // (2 * fmt[1])
        pos = body + size + (size & 1)  # chunks are padded to an even size
    raise KaldiFormatError(f"{what}: no data chunk")


def _wav_channel(buf, body, frames, channels, channel, what):
    if not 0 <= channel < channels:
        raise KaldiFormatError(f"{what}: channel {channel} of a file with {channels}")
    return np.frombuffer(buf, dtype="<i2", count=frames * channels, offset=body)[channel::channels]


def _is_pipe(rx):
    return rx.rstrip().endswith("|")


def read_wav(f, channel=0):
    """A wave file (path, or 'path:offset' as an scp names it) -> (sample_rate, int16 array of one channel).  RIFF/WAVE with
    format tag 1 or the extensible header with the PCM sub-format, 16 bits per sample, any number of channels; other chunks
    are skipped; a data size of 0 or 0xFFFFFFFF means to the end of the file.  The file is memory-mapped."""
    f = os.fspath(f)
    if _is_pipe(f):
        raise KaldiFormatError(f"{f}: command pipes are not read")
    path, off = _split_rx(f)
    buf = np.memmap(path, dtype=np.uint8, mode="r")
    rate, ch, body, frames = _wav_layout(buf, off or 0, path)
    return rate, np.array(_wav_channel(buf, body, frames, ch, channel, path), dtype=np.int16)


def write_wav(path, samples, sample_frequency):
    """A 16-bit mono RIFF/WAVE file (format tag 1, a 44-byte header) that read_wav reads back; samples: int16."""
    x = np.asarray(samples)
    if x.dtype != np.int16 or x.ndim != 1:
        raise ValueError("write_wav: expected a one-dimensional int16 array")
    rate, nbytes = int(sample_frequency), 2 * int(x.shape[0])
    if rate < 1 or nbytes + 36 > 0xFFFFFFFF:
        raise ValueError(f"write_wav: sample rate {rate}, {nbytes} bytes of samples")
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 36 + nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) +
                 b"data" + struct.pack("<I", nbytes))
        fh.write(x.astype("<i2").tobytes())


def load_wav_scp(path, entries=None, sample_frequency=None, channel=0, return_rates=False):
    """Kaldi wav.scp -> (keys, offsets int64 (U + 1), samples int16): the chosen channel of every file, one after the other
    in ONE buffer; utterance u is samples[offsets[u]:offsets[u + 1]].  `entries`: a slice of read_scp(path) to load instead
    of the whole file.  An entry that is a command pipe (ends in `|`), a file that is not 16-bit PCM, a truncated data
    chunk, or (if given) a sample rate other than sample_frequency is a KaldiFormatError naming the key.  `segments` files
    are not read.  return_rates: a fourth result, the (U,) int64 sample rates of the files (with sample_frequency=None files
    of any rate are loaded: neuralplda_amd.resample brings them to one)."""
    if entries is None:
        entries = read_scp(path)
    layout, offsets, rates = [], np.zeros(len(entries) + 1, dtype=np.int64), np.zeros(len(entries), dtype=np.int64)
    for i, (key, rx) in enumerate(entries):
        if _is_pipe(rx):
            raise KaldiFormatError(f"{key}: command pipes in a wav.scp are not read ({rx.strip()!r})")
        f, off = _split_rx(rx)
        try:
            buf = np.memmap(_scp_file(f, path), dtype=np.uint8, mode="r")
        except (OSError, ValueError) as e:
            raise KaldiFormatError(f"{key}: cannot map {f}: {e}") from None
        rate, ch, body, frames = _wav_layout(buf, off or 0, key)
        if sample_frequency is not None and rate != int(sample_frequency):
            raise KaldiFormatError(f"{key}: sample rate {rate}, expected {int(sample_frequency)} (there is no resampling)")
        layout.append(_wav_channel(buf, body, frames, ch, channel, key))
        offsets[i + 1], rates[i] = offsets[i] + frames, rate
    samples = np.empty(int(offsets[-1]), dtype=np.int16)
    for i, src in enumerate(layout):
        samples[offsets[i]:offsets[i + 1]] = src
    keys = [k for k, _ in entries]
    return (keys, offsets, samples, rates) if return_rates else (keys, offsets, samples)


# ---- Kaldi initialisation of the model classes --------------------------------------------------------------------

def fold_init(model, mean_vec_file, transform_mat_file, plda_file=None):
    """Write a Kaldi LDA (+ PLDA) into a model's parameters the way the reference's loaders do
    (NeuralPlda.LoadPldaParamsFromKaldi utils/models.py:441-457, DPlda.LoadParamsFromKaldi :551-564,
    GaussianBackend.LoadPldaParamsFromKaldi :653-658), reading the files natively:
      centering_and_LDA            <- T[:, :-1],  T[:, -1] - T[:, :-1] mean           (mean subtraction folded into the bias)
      centering_and_wccn_plda      <- D,  -D plda_mean                                 (only with a PLDA file)
      P_sqrt, Q                    <- sqrt(diagP), diagQ of plda_psi_to_pq(Psi)
    The parameters are written through `.data` like the reference does and their version counters are bumped, so cached
    parameter images are rebuilt."""
    plda = None
    if plda_file is not None:
        d = read_plda(plda_file)
        plda = (d["plda_mean"], d["diagonalizing_transform"], d["Psi_across_covar_diag"])
    fold_arrays(model, read_vector(mean_vec_file), read_matrix(transform_mat_file), plda)


def fold_arrays(model, mean_vec, transform_mat, plda=None):
    """The array-level half of fold_init: mean_vec (D0), transform_mat (D1, D0 + 1) and optionally plda = (plda_mean,
    diagonalizing transform, Psi) as arrays — what the files hold, or what neuralplda_amd.backend estimated."""
    import torch
    T = np.asarray(transform_mat, dtype=np.float64)
    mean = np.asarray(mean_vec, dtype=np.float64)
    new = {"centering_and_LDA.weight": T[:, :-1], "centering_and_LDA.bias": T[:, -1] - T[:, :-1].dot(mean)}
    if plda is not None:
        plda_mean, D, psi = (np.asarray(a, dtype=np.float64) for a in plda)
        diagP, diagQ = plda_psi_to_pq(psi)
        new.update({"centering_and_wccn_plda.weight": D, "centering_and_wccn_plda.bias": -D.dot(plda_mean),
                    "P_sqrt": np.sqrt(diagP), "Q": diagQ})
    sd = model.state_dict()
    for name, val in new.items():
        sd[name].data.copy_(torch.from_numpy(np.ascontiguousarray(val)).float())
    params = dict(model.named_parameters())
    for name in new:
        if name in params:
            torch.autograd.graph.increment_version(params[name])


# ---- writers (used by tests and by tools that synthesise Kaldi-format fixtures) -----------------

def _bin_vec(v, double):
    v = np.asarray(v)
    dt, tok = ("<f8", b"DV ") if double else ("<f4", b"FV ")
    return tok + b"\x04" + struct.pack("<i", v.shape[0]) + v.astype(dt).tobytes()


def _bin_mat(m, double):
    m = np.asarray(m)
    dt, tok = ("<f8", b"DM ") if double else ("<f4", b"FM ")
    return tok + b"\x04" + struct.pack("<i", m.shape[0]) + b"\x04" + struct.pack("<i", m.shape[1]) + \
        np.ascontiguousarray(m).astype(dt).tobytes()


def write_vector_binary(path, v, double=False):
    with open(path, "wb") as fh:
        fh.write(b"\0B" + _bin_vec(v, double))


def write_matrix_binary(path, m, double=False):
    with open(path, "wb") as fh:
        fh.write(b"\0B" + _bin_mat(m, double))


def write_feature_ark(ark_path, keys, mats, scp_path=None):
    """Binary float-matrix archive 'key \\0BFM ...' per matrix (what copy-feats writes uncompressed), optionally with the
    matching scp.  -> the offsets of the \\0B markers."""
    if len(keys) != len(mats):
        raise ValueError("one key per matrix")
    offsets, pos = [], 0
    with open(ark_path, "wb") as fh:
        for k, m in zip(keys, mats):
            kb = k.encode("ascii") + b" "
            m = np.asarray(m, dtype=np.float32)
            if m.ndim != 2:
                raise ValueError(f"{k}: expected a (frames, columns) matrix")
            obj = kb + b"\0B" + _bin_mat(m, False)
            offsets.append(pos + len(kb))
            fh.write(obj)
            pos += len(obj)
    if scp_path is not None:
        with open(scp_path, "w") as fh:
            fh.write("".join(f"{k} {ark_path}:{o}\n" for k, o in zip(keys, offsets)))
    return offsets


def write_plda_binary(path, mean, transform, psi):
    with open(path, "wb") as fh:
        fh.write(b"\0B<Plda> " + _bin_vec(mean, True) + _bin_mat(transform, True) + _bin_vec(psi, True) +
                 b"</Plda> ")
