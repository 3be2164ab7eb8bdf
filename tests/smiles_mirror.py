"""CPU yardstick of ``dsl_smiles_records`` (include/diffspectra_smiles.h), in plain Python: the written graph, the canonical order (colour
refinement with individualisation, the signature order of the header restated with Python integers), the writer, and a parser of the same
SMILES subset that shares no code with the writer and expands implied and bracket hydrogens back into a molecule dict, so that
``graph_mirror.same_graph(parse(write(m)), m)`` is a statement about both.  A molecule is the dict of ``structure_mirror.mol_from_record``.

Also here: the strings that the definition forces whatever the signature order is (``forced_table``) and the molecules of the property
checks (``property_molecules``), which tests/test_smiles_cpu.py and tests/test_smiles_gpu.py share."""
from __future__ import annotations

import functools

import numpy as np

from tests import graph_mirror as GM, structure_mirror as SM

W = SM.W
MASK = (1 << 64) - 1
OK, UNCERTIFIED, OVERFLOW, UNUSABLE = 0, 1, 2, 3
TEXT_BYTES = 384
MAX_RINGS = 99
SYMBOLS = "HCNOF"
VALENCES = {1: (4,), 2: (3, 5), 3: (2,), 4: (1,)}
KEYS = ("text", "length", "status", "nodes", "atom_order")


# ------------------------------------------------------------------------------------------------------------------ the written graph

def written_graph(mol):
    """(atoms, label, bond): the record indices of the written atoms in ascending order, ``label[i] = (type, charge byte, folded hydrogens)``
    and the symmetric bond bytes over record indices with every bond of a folded hydrogen set to 0."""
    n = len(mol["type"])
    A = GM._adjacency(mol)
    typ = [int(t) for t in mol["type"]]
    fc = [int(c) & 255 for c in mol["fc"]]
    folded = [False] * n
    for i in range(n):
        nb = [j for j in range(n) if A[i][j]]
        folded[i] = typ[i] == 0 and fc[i] == 0 and len(nb) == 1 and A[i][nb[0]] == 1 and typ[nb[0]] != 0
    h = [sum(1 for j in range(n) if A[i][j] and folded[j]) for i in range(n)]
    for i in range(n):
        if folded[i]:
            for j in range(n):
                A[i][j] = A[j][i] = 0
    return [i for i in range(n) if not folded[i]], [(typ[i], fc[i], h[i]) for i in range(n)], A


# ------------------------------------------------------------------------------------------------------------------ the canonical order

def _refine(colour, atoms, A):
    """The stable colouring below ``colour`` (dict atom -> colour): signature = colour * 2^58 + (sum over bonded written neighbours of
    fmix(neighbour colour + 1) * (2 bond + 1) mod 2^64) >> 6, new colour = atoms with a smaller signature; until the cells stop growing."""
    classes = 0
    while True:
        f = {i: GM.fmix(colour[i] + 1) for i in atoms}
        sig = {i: (colour[i] << 58) | ((sum(f[j] * (2 * A[i][j] + 1) for j in atoms if A[i][j]) & MASK) >> 6) for i in atoms}
        colour = {i: sum(1 for j in atoms if sig[j] < sig[i]) for i in atoms}
        now = len(set(sig.values()))
        if now == classes:
            return colour
        classes = now


def canonical_order(mol, max_nodes=4096):
    """(position of every written atom or None, status OK / UNCERTIFIED, nodes)."""
    atoms, label, A = written_graph(mol)
    key = {i: (4 - label[i][0]) << 16 | label[i][1] << 8 | label[i][2] for i in atoms}      # F, O, N, C, H: the header's label key
    first = _refine({i: sum(1 for j in atoms if key[j] < key[i]) for i in atoms}, atoms, A)
    state = dict(nodes=0, best=None, cert=None, stopped=False)

    def leaf(colour):
        inv = sorted(atoms, key=lambda i: colour[i])
        cert = [A[inv[p]][inv[q]] for p in range(len(inv)) for q in range(p + 1, len(inv))]
        if state["best"] is None or cert < state["cert"]:
            state["best"], state["cert"] = dict(colour), cert

    def search(colour):
        cells = {}
        for i in atoms:
            cells.setdefault(colour[i], []).append(i)
        multi = sorted(c for c, members in cells.items() if len(members) > 1)
        if not multi:
            leaf(colour)
            return
        c, tried = multi[0], []
        for u in cells[c]:
            if any(all(A[u][k] == A[v][k] for k in atoms if k != u and k != v) for v in tried):
                continue
            if state["best"] is not None and state["nodes"] >= max_nodes:
                state["stopped"] = True
                return
            state["nodes"] += 1
            tried.append(u)
            search(_refine({i: colour[i] + (1 if colour[i] == c and i != u else 0) for i in atoms}, atoms, A))
            if state["stopped"]:
                return

    if atoms:
        search(first)
    return state["best"], (UNCERTIFIED if state["stopped"] else OK), state["nodes"]


def refinement_is_discrete(mol):
    """Colour refinement alone orders the written atoms: the search needs no individualisation."""
    atoms, label, A = written_graph(mol)
    key = {i: (4 - label[i][0]) << 16 | label[i][1] << 8 | label[i][2] for i in atoms}
    colour = _refine({i: sum(1 for j in atoms if key[j] < key[i]) for i in atoms}, atoms, A)
    return len(set(colour.values())) == len(atoms)


# ------------------------------------------------------------------------------------------------------------------ the writer

def _number(k):
    return str(k) if k < 10 else "%%%02d" % k


def _atom_text(label, bond_sum):
    t, c, h = label
    c = c - 256 if c > 127 else c
    implied = 0
    for v in VALENCES.get(t, ()):
        if v >= bond_sum:
            implied = v - bond_sum
            break
    if t != 0 and c == 0 and h == implied:
        return SYMBOLS[t]
    hs = "" if h == 0 else "H" if h == 1 else "H%d" % h
    cs = "" if c == 0 else ("+" if c > 0 else "-") + ("" if abs(c) == 1 else str(abs(c)))
    return "[" + SYMBOLS[t] + hs + cs + "]"


class _Overflow(Exception):
    pass


def _write(atoms, label, A, position):
    """The string of the written graph under ``position`` and the visit index of every written atom."""
    m = len(atoms)
    inv = sorted(atoms, key=lambda i: position[i])
    B = [[A[inv[p]][inv[q]] for q in range(m)] for p in range(m)]
    vis, parent, order = [-1] * m, [-1] * m, []

    def visit(a):
        vis[a] = len(order)
        order.append(a)
        for b in range(m):
            if B[a][b] and vis[b] < 0:
                parent[b] = a
                visit(b)
    roots = []
    for p in range(m):
        if vis[p] < 0:
            roots.append(p)
            visit(p)
    ring = lambda a, b: B[a][b] and parent[a] != b and parent[b] != a
    slot = {}                                    # number -> (opening atom, partner)
    symbol = {1: "", 2: "=", 3: "#"}

    def emit(a):
        out = [_atom_text(label[inv[a]], sum(B[a]))]
        released = []
        for b in order[:vis[a]]:
            if ring(a, b):
                k = next(k for k, v in slot.items() if v == (b, a))
                out.append(_number(k))
                released.append(k)
        for b in order[vis[a] + 1:]:
            if ring(a, b):
                k = next((k for k in range(1, MAX_RINGS + 1) if k not in slot), None)
                if k is None:
                    raise _Overflow
                slot[k] = (a, b)
                out.append(symbol[B[a][b]] + _number(k))
        for k in released:
            del slot[k]
        children = [b for b in range(m) if parent[b] == a]
        for b in children:
            inner = symbol[B[a][b]] + emit(b)
            out.append(inner if b == children[-1] else "(" + inner + ")")
        return "".join(out)
    text = ".".join(emit(r) for r in roots)
    return text, {inv[a]: vis[a] for a in range(m)}


def write(mol, max_nodes=4096):
    """One row of ``dsl_smiles_records`` as a dict: ``text`` (bytes), ``length``, ``status``, ``nodes``, ``atom_order`` (29 ints)."""
    n = len(mol["type"])
    none = dict(text=b"", length=0, status=UNUSABLE, nodes=0, atom_order=[-1] * W)
    A = GM._adjacency(mol)
    if n == 0 or n > W or any(int(t) > 4 or int(t) < 0 for t in mol["type"]) or any(A[i][j] > 3 for i in range(n) for j in range(n)):
        return none
    atoms, label, A = written_graph(mol)
    position, status, nodes = canonical_order(mol, max_nodes)
    try:
        text, vis = _write(atoms, label, A, position)
        if len(text) > TEXT_BYTES:
            raise _Overflow
    except _Overflow:
        return dict(none, status=OVERFLOW, nodes=nodes)
    return dict(text=text.encode("ascii"), length=len(text), status=status, nodes=nodes, atom_order=[vis.get(i, -1) for i in range(W)])


def write_record(rec, n, max_nodes=4096):
    n = int(min(max(int(n), 0), W))
    return write(SM.mol_from_record(rec, n) if n else dict(type=[], fc=[], bond=np.zeros((0, 0))), max_nodes)


def write_table(rec, n, max_nodes=4096):
    return [write_record(r, k, max_nodes) for r, k in zip(rec, n)]


def smiles(mol, max_nodes=4096):
    row = write(mol, max_nodes)
    return row["text"].decode("ascii") if row["status"] in (OK, UNCERTIFIED) else None


# ------------------------------------------------------------------------------------------------------------------ the parser

def parse(text):
    """Molecule dict of a string of the subset: the atoms of the string in their order, then every hydrogen that a bracket or a bare symbol
    implies, one after the other, behind the atom that carries it."""
    elements = {"H": 0, "C": 1, "N": 2, "O": 3, "F": 4}
    order_of = {"=": 2, "#": 3}
    normal = {1: [4], 2: [3, 5], 3: [2], 4: [1]}
    atoms, bonds, stack, opened = [], {}, [], {}
    last, pending, at = None, 1, 0
    while at < len(text):
        ch = text[at]
        if ch == "[":
            end = text.index("]", at)
            body = text[at + 1:end]
            el, rest = body[0], body[1:]
            h = charge = 0
            if rest.startswith("H"):
                digits = ""
                rest = rest[1:]
                while rest and rest[0].isdigit():
                    digits, rest = digits + rest[0], rest[1:]
                h = int(digits) if digits else 1
            if rest:
                sign, size = rest[0], rest[1:]
                assert sign in "+-" and (size == "" or size.isdigit()), text
                charge = (1 if sign == "+" else -1) * (int(size) if size else 1)
            atoms.append([elements[el], charge, h])
            at = end + 1
        elif ch in elements and ch != "H":
            atoms.append([elements[ch], 0, None])
            at += 1
        elif ch in order_of:
            pending = order_of[ch]
            at += 1
            continue
        elif ch == "(":
            stack.append(last)
            at += 1
            continue
        elif ch == ")":
            last = stack.pop()
            at += 1
            continue
        elif ch == ".":
            last, pending = None, 1
            assert not stack, text
            at += 1
            continue
        elif ch.isdigit() or ch == "%":
            k, at = (int(text[at + 1:at + 3]), at + 3) if ch == "%" else (int(ch), at + 1)
            if k in opened:
                other, order = opened.pop(k)
                assert pending == 1 and (other, last) not in bonds, text
                bonds[(other, last)] = order
            else:
                opened[k] = (last, pending)
            pending = 1
            continue
        else:
            raise ValueError(f"{text!r}: character {ch!r}")
        new = len(atoms) - 1
        if last is not None:
            bonds[(last, new)] = pending
        last, pending = new, 1
    assert not opened and not stack, text
    total = [0] * len(atoms)
    for (i, j), o in bonds.items():
        total[i] += o
        total[j] += o
    types, fc, edges, orders = [a[0] for a in atoms], [a[1] for a in atoms], list(bonds), list(bonds.values())
    for i, (t, _, h) in enumerate(atoms):
        if h is None:
            room = [v for v in normal[t] if v >= total[i]]
            h = room[0] - total[i] if room else 0
        for _ in range(h):
            edges.append((i, len(types)))
            orders.append(1)
            types.append(0)
            fc.append(0)
    mol = GM.molecule(types, edges, fc=fc, orders=orders)
    mol["string_atoms"] = len(atoms)
    return mol


def expanded_order(mol, atom_order):
    """``atom_order`` of a row continued over the folded hydrogens in the way ``parse`` appends them: a map of every record atom onto the
    atoms of ``parse(text)``, to be checked with ``graph_mirror.is_isomorphism``."""
    atoms, label, A = written_graph(mol)
    full = GM._adjacency(mol)
    n = len(mol["type"])
    image = [int(atom_order[i]) for i in range(n)]
    nxt = len(atoms)
    for a in sorted(atoms, key=lambda i: image[i]):
        for j in range(n):
            if full[a][j] and image[j] < 0:
                image[j] = nxt
                nxt += 1
    return image


# ------------------------------------------------------------------------------------------------------------------ molecules

def _mol(types, edges=(), orders=None, fc=None):
    return GM.molecule(types, list(edges), fc=fc, orders=orders)


def _with_h(types, edges, orders, counts, fc=None):
    """Heavy atoms plus ``counts[i]`` hydrogens on atom i."""
    types, edges, orders = list(types), list(edges), list(orders)
    fc = list(fc) if fc is not None else [0] * len(types)
    for i, k in enumerate(counts):
        for _ in range(k):
            edges.append((i, len(types)))
            orders.append(1)
            types.append(0)
            fc.append(0)
    return _mol(types, edges, orders, fc)


def forced_table():
    """[(string, molecule)]: what the definition forces whatever the signature order is."""
    H = lambda types, edges, orders, counts, fc=None: _with_h(types, edges, orders, counts, fc)
    return [
        ("C", H([1], [], [], [4])), ("O", H([3], [], [], [2])), ("F", H([4], [], [], [1])), ("N", H([2], [], [], [3])),
        ("[NH4+]", H([2], [], [], [4], [1])), ("[OH-]", H([3], [], [], [1], [-1])), ("[CH3]", H([1], [], [], [3])), ("[CH2]", H([1], [], [], [2])),
        ("[H][H]", _mol([0, 0], [(0, 1)])), ("[H]", _mol([0])), ("[H+]", _mol([0], fc=[1])),
        ("CC", H([1, 1], [(0, 1)], [1], [3, 3])), ("C=C", H([1, 1], [(0, 1)], [2], [2, 2])), ("C#C", H([1, 1], [(0, 1)], [3], [1, 1])),
        ("N#N", _mol([2, 2], [(0, 1)], [3])), ("O=C=O", _mol([3, 1, 3], [(0, 1), (1, 2)], [2, 2])), ("FF", _mol([4, 4], [(0, 1)])),
        ("O.O", H([3, 3], [], [], [2, 2])), ("C1CC1", H([1, 1, 1], [(0, 1), (1, 2), (0, 2)], [1, 1, 1], [2, 2, 2])),
    ]


def ring_of(k, start=0):
    return [(start + i, start + (i + 1) % k) for i in range(k)]


def benzene(shift=0):
    return _with_h([1] * 6, ring_of(6), [2 if (i + shift) % 2 == 0 else 1 for i in range(6)], [1] * 6)


def methylpyridine(shift=0):
    """2-methylpyridine, N = atom 0, the methyl on atom 1; the two Kekule drawings (no symmetry maps one onto the other)."""
    return _with_h([2, 1, 1, 1, 1, 1, 1], ring_of(6) + [(1, 6)], [2 if (i + shift) % 2 == 0 else 1 for i in range(6)] + [1], [0, 0, 1, 1, 1, 1, 3])


def glycine_zwitterion():
    """[NH3+]CC(=O)[O-]"""
    return _with_h([2, 1, 1, 3, 3], [(0, 1), (1, 2), (2, 3), (2, 4)], [1, 1, 2, 1], [3, 2, 0, 0, 0], [1, 0, 0, 0, -1])


def bridging_hydrogen():
    """A hydrogen between two carbons (a written atom: two bonds), each carbon with two hydrogens of its own."""
    return _with_h([1, 1, 0], [(0, 2), (1, 2)], [1, 1], [2, 2, 0])


def cubane():
    return GM.saturated(GM.hard_pairs()[3][1])


def propane():
    return GM.saturated(GM.carbons(3, [(0, 1), (1, 2)]))


def tetra_tert_butyl_methane():
    edges = [(0, 1 + k) for k in range(4)] + [(1 + k, 5 + 3 * k + j) for k in range(4) for j in range(3)]
    return GM.carbons(17, edges)


def ring29():
    return GM.carbons(29, ring_of(29))


def stacked_rings():
    return GM.carbons(20, ring_of(10) + ring_of(10, 10) + [(i, 10 + i) for i in range(10)])


@functools.lru_cache(maxsize=1)
def property_molecules():
    """[(name, molecule)] of the property checks, the seeded pairs apart."""
    out = []
    for name, a, b in GM.hard_pairs():
        out += [(name + " / a", a), (name + " / b", b)]
    out += [("nonane", GM.nonane()), ("k29", GM.k29()), ("29 carbons", GM.carbons(29, [])), ("29-ring", ring29()),
            ("tetra-tert-butyl-methane", tetra_tert_butyl_methane()), ("cubane", cubane()), ("benzene a", benzene(0)), ("benzene b", benzene(1)),
            ("2-methylpyridine a", methylpyridine(0)), ("2-methylpyridine b", methylpyridine(1)), ("glycine zwitterion", glycine_zwitterion()),
            ("bridging hydrogen", bridging_hydrogen()), ("stacked 10-rings", stacked_rings())]
    return out


@functools.lru_cache(maxsize=2)
def seeded_rows(count=2000):
    """The mirror's rows of both sides of ``graph_mirror.seeded_pairs(count)``: (ref rows, generated rows), computed once."""
    ref, prb, _ = GM.seeded_pairs(count)
    return [write(m) for m in ref], [write(m) for m in prb]
