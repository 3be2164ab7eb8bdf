"""Plain Python / numpy mirror of ``ds_geometry_count_records`` / ``ds_geometry_fill_records`` and ``ds_mmd_1d_segments``, written from the text
of include/diffspectra_hip.h: the enumeration of bonds, angles and dihedrals in the header's order, their values in fp64 (every product and
sum rounded on its own, as numpy's elementwise operations do), the class match up to reversal, and the MMD of the reference's formula in fp64
over all pairs.  Molecules are the dicts of tests/structure_mirror.py (``pos``, ``type``, ``fc``, ``bond``)."""
import numpy as np

DEG = 180.0 / np.pi
KINDS = ("bond", "angle", "dihedral")


def neighbours(mol):
    """N(i) of every atom, ascending: the upper triangle of the bond matrix decides, as bytes."""
    n = len(mol["type"])
    b = np.asarray(mol["bond"]).astype(np.int64) & 255
    order = [[int(b[min(i, j), max(i, j)]) if i != j else 0 for j in range(n)] for i in range(n)]
    return [[j for j in range(n) if order[i][j] > 0] for i in range(n)], order


def entries(mol):
    """Every bond, angle and dihedral of the molecule in the header's order -> three lists of (fields, atoms).  ``fields`` alternate type
    byte and bond byte along ``atoms``."""
    nb, order = neighbours(mol)
    t = [int(x) & 255 for x in mol["type"]]
    n = len(t)
    bonds, angles, dihedrals = [], [], []
    for i in range(n):
        for j in nb[i]:
            if j > i:
                bonds.append(((t[i], order[i][j], t[j]), (i, j)))
    for c in range(n):
        for a in nb[c]:
            for b in nb[c]:
                if b > a:
                    angles.append(((t[a], order[a][c], t[c], order[c][b], t[b]), (a, c, b)))
    for i in range(n):
        for j in nb[i]:
            if j > i:
                for a in nb[i]:
                    if a != j:
                        for b in nb[j]:
                            if b != i:
                                dihedrals.append(((t[a], order[a][i], t[i], order[i][j], t[j], order[j][b], t[b]), (a, i, j, b)))
    return bonds, angles, dihedrals


def code_fields(code, groups):
    return tuple((int(code) >> (4 * k)) & 15 for k in range(groups))


def class_lookup(codes, groups):
    """{fields: position of the first class whose code is ``fields`` forwards or backwards}; a field above 15 is in no key."""
    table = {}
    for k, code in enumerate(codes):
        if code < 0 or int(code) >> (4 * groups):
            continue
        f = code_fields(code, groups)
        table.setdefault(f, k)
        table.setdefault(f[::-1], k)
    return table


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)


def bond_values(pos, atoms):
    """(value f64, defined) of bonds ``atoms [K, 2]``."""
    d = pos[atoms[:, 0]] - pos[atoms[:, 1]]
    s = _dot(d, d)
    with np.errstate(all="ignore"):
        v = np.sqrt(s)
    return v, (s > 0) & np.isfinite(v)


def angle_values(pos, atoms):
    """(degrees f64, defined) of angles ``atoms [K, 3]`` = (a, c, b)."""
    with np.errstate(all="ignore"):
        u, v = pos[atoms[:, 0]] - pos[atoms[:, 1]], pos[atoms[:, 2]] - pos[atoms[:, 1]]
        den = np.sqrt(_dot(u, u) * _dot(v, v))
        ok = (den > 0) & np.isfinite(den)
        cs = np.minimum(np.maximum(_dot(u, v) / np.where(ok, den, 1.0), -1.0), 1.0)
        deg = np.arccos(cs) * DEG
    return deg, ok & np.isfinite(deg)


def dihedral_values(pos, atoms):
    """(degrees f64 as atan2 gives them, defined) of dihedrals ``atoms [K, 4]`` = (a, i, j, b)."""
    with np.errstate(all="ignore"):
        b1, b2, b3 = pos[atoms[:, 1]] - pos[atoms[:, 0]], pos[atoms[:, 2]] - pos[atoms[:, 1]], pos[atoms[:, 3]] - pos[atoms[:, 2]]
        n1, n2 = _cross(b1, b2), _cross(b2, b3)
        b2b2 = _dot(b2, b2)
        ok = (_dot(n1, n1) > 0) & (_dot(n2, n2) > 0) & (b2b2 > 0)
        y = _dot(_cross(n1, n2), b2) / np.sqrt(np.where(ok, b2b2, 1.0))
        deg = np.arctan2(y, _dot(n1, n2)) * DEG
    return deg, ok & np.isfinite(deg)


def to_f32(kind, deg):
    """The one rounding to fp32; a dihedral that rounds to <= -180 becomes +180."""
    v = np.asarray(deg, np.float64).astype(np.float32)
    if kind == 2:
        v = np.where(v <= np.float32(-180.0), np.float32(180.0), v)
    return v


VALUE_FNS = (bond_values, angle_values, dihedral_values)


def extract(mol, codes):
    """What the two kernels give for one record: per kind ``(value64 [K], value32 [K], cls [K], atoms [K, 2|3|4])`` of the emitted entries in
    the header's order, and ``skipped``.  ``codes``: the three class tables (lists of ints).  Positions are the record's fp32 values."""
    pos = np.asarray(mol["pos"], np.float32).astype(np.float64).reshape(-1, 3)
    out, skipped = [], 0
    for kind, (found, table) in enumerate(zip(entries(mol), codes)):
        groups = 3 + 2 * kind
        lookup = class_lookup(table, groups)
        listed = [(lookup[f], a) for f, a in found if max(f) <= 15 and f in lookup]
        atoms = np.array([a for _, a in listed], np.int64).reshape(-1, kind + 2)
        cls = np.array([k for k, _ in listed], np.int64)
        v, ok = VALUE_FNS[kind](pos, atoms)
        skipped += int((~ok).sum())
        out.append((v[ok], to_f32(kind, v[ok]), cls[ok], atoms[ok]))
    return out, skipped


def by_class(values, cls, n_classes):
    return [values[cls == k] for k in range(n_classes)]


def mmd(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """(mmd, XX, YY, XY, bandwidth) of the header's definition in fp64 over all pairs; NaNs for an empty side or a zero bandwidth."""
    x, y = np.asarray(source, np.float64).reshape(-1), np.asarray(target, np.float64).reshape(-1)
    ns, nt = len(x), len(y)
    nan = float("nan")
    if ns == 0 or nt == 0:
        return (nan,) * 5
    z = np.concatenate([x, y])
    N = ns + nt
    d2 = (z[:, None] - z[None, :]) ** 2
    bandwidth = float(fix_sigma) if fix_sigma else float(d2.sum() / (N * N - N))
    if not bandwidth > 0 or not np.isfinite(bandwidth):
        return nan, nan, nan, nan, bandwidth
    bw = bandwidth / kernel_mul ** (kernel_num // 2)
    k = sum(np.exp(-d2 / (bw * kernel_mul ** i)) for i in range(kernel_num))
    xx, yy, xy = k[:ns, :ns].sum() / (ns * ns), k[ns:, ns:].sum() / (nt * nt), k[:ns, ns:].sum() / (ns * nt)
    return float(xx + yy - 2 * xy), float(xx), float(yy), float(xy), bandwidth


def symbol(fields, decoder=("H", "C", "N", "O", "F")):
    """(1, 1, 0) -> 'C1H'; (0, 1, 1, 1, 2) -> 'H1C-C1N': the reference's way of writing a class."""
    parts = [decoder[fields[k]] + str(fields[k + 1]) + decoder[fields[k + 2]] for k in range(0, len(fields) - 2, 2)]
    return "-".join(parts)
