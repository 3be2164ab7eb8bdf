"""CPU yardstick of ``dsp_read_smiles`` (include/diffspectra_reader.h), in plain Python and written from the header: a serial tokenizer with an
explicit stack, the ring-bond test, the depth-first Kekule search, the hydrogens and the record.  It shares no code with
``tests/smiles_mirror.parse`` (the test helper of the writer's subset) and returns the kernel's fields byte for byte.

Also here: (a) ``hand_table`` - strings with molecules stated by hand, (b) ``error_table`` - strings with hand-stated ``(status, where)``,
(c) ``generated`` - a seeded generator of valid strings that counts its atoms and hydrogens as it builds, and ``edited`` - random single-byte
edits of them.  tests/test_smiles_reader_cpu.py pins the mirror to (a) and (b); tests/test_smiles_reader_gpu.py compares the kernel with it."""
from __future__ import annotations

import functools

import numpy as np

W = 29
RECORD_BYTES = 1248
TYPE, FC, BOND = 348, 377, 406          # byte offsets of a record's fields (plain numbers, as in tests/structure_mirror.py)
TEXT_BYTES = 384
OK, EMPTY, SYNTAX, ELEMENT, KEKULE, TOO_LARGE, UNDECIDED, TOO_LONG = range(8)
STATUS_NAMES = ("ok", "empty", "syntax", "element", "kekule", "too large", "undecided", "too long")
F_ISOTOPE, F_CHIRAL, F_DIRECTION, F_CLASS, F_AROMATIC = 1, 2, 4, 8, 16
FIELDS = ("rec", "n", "status", "where", "string_atoms", "flags", "aromatic", "atom_pos", "nodes")
ELEMENTS = {"H": 0, "C": 1, "N": 2, "O": 3, "F": 4}
SOFT = 4                                # the code of ':' and, with 0, of an unwritten bond: aromatic or single, decided by the graph


class _Stop(Exception):
    def __init__(self, status, where):
        self.status, self.where = status, where


class _Unclosed(Exception):
    """The text ended inside the bracket atom that opened at ``where``."""
    def __init__(self, where):
        self.where = where


def _digit(c):
    return 48 <= c <= 57


def _lower(c):
    return 97 <= c <= 122


def _upper(c):
    return 65 <= c <= 90


def _bracket(t, at, flags):
    """The bracket atom whose '[' stands at ``at``: (atom, index after ']', flags)."""
    L, i = len(t), at + 1

    def peek():
        if i >= L:
            raise _Unclosed(at)
        return t[i]
    if _digit(peek()):
        flags |= F_ISOTOPE
        while _digit(peek()):
            i += 1
    c = peek()
    if _upper(c):
        two = i + 1 < L and _lower(t[i + 1])
        if two or chr(c) not in ELEMENTS:
            raise _Stop(ELEMENT, i)
        typ, arom = ELEMENTS[chr(c)], False
    elif chr(c) in "cno":
        typ, arom = ELEMENTS[chr(c).upper()], True
    elif chr(c) in "bsp*":
        raise _Stop(ELEMENT, i)
    else:
        raise _Stop(SYNTAX, i)
    pos = i
    i += 1
    if peek() == 64:                    # '@', '@@'
        flags |= F_CHIRAL
        i += 1
        if peek() == 64:
            i += 1
    h = 0
    if peek() == 72:                    # 'H', 'Hd'
        h = 1
        i += 1
        if _digit(peek()):
            h = t[i] - 48
            i += 1
    charge = 0
    if peek() in (43, 45):              # '+', '-', '++', '--', sign and 1..3 digits
        sign_at, sign = i, 1 if t[i] == 43 else -1
        i += 1
        if peek() == t[sign_at]:
            charge = 2 * sign
            i += 1
        elif _digit(peek()):
            size, digits = 0, 0
            while digits < 3 and _digit(peek()):
                size, digits, i = size * 10 + t[i] - 48, digits + 1, i + 1
            if size > 127:
                raise _Stop(SYNTAX, sign_at)
            charge = sign * size
        else:
            charge = sign
    if peek() == 58:                    # ':' and digits
        flags |= F_CLASS
        i += 1
        if not _digit(peek()):
            raise _Stop(SYNTAX, i)
        while _digit(peek()):
            i += 1
    if peek() != 93:
        raise _Stop(SYNTAX, i)
    return dict(type=typ, charge=charge, h=h, arom=arom, pos=pos), i + 1, flags


def _scan(t):
    """The tokenizer: (atoms, bonds [(a, b, code)], flags) or _Stop."""
    L = len(t)
    atoms, bonds, stack, ring = [], [], [], {}
    flags, last, pending = 0, -1, 0
    need, need_kind = -1, ""                    # the token that asks for an atom: a bond symbol, '(' or '.'
    unclosed = None
    i = 0
    while i < L:
        c = t[i]
        ch = chr(c) if c < 128 else "\xff"
        atom = None
        if ch == "[":
            try:
                atom, nxt, flags = _bracket(t, i, flags)
            except _Unclosed as u:
                unclosed, need = u.where, -1
                break
            start = i
        elif ch in "CNOFcno":
            if ch == "C" and i + 1 < L and t[i + 1] == 108:          # Cl
                raise _Stop(ELEMENT, i)
            atom, nxt, start = dict(type=ELEMENTS[ch.upper()], charge=0, h=None, arom=ch.islower(), pos=i), i + 1, i
        elif ch in "BSPIbsp*":
            raise _Stop(ELEMENT, i)
        elif ch in "-=#:/\\":
            if pending or last < 0 or need_kind == ".":
                raise _Stop(SYNTAX, i)
            if ch in "/\\":
                flags |= F_DIRECTION
            pending = {"-": 1, "=": 2, "#": 3, ":": SOFT, "/": 1, "\\": 1}[ch]
            need, need_kind = i, "(" if need_kind == "(" else "b"       # after '(' and a bond symbol an atom must follow, no ring number
            i += 1
            continue
        elif ch.isdigit() or ch == "%":
            if ch == "%":
                if not (i + 2 < L and _digit(t[i + 1]) and _digit(t[i + 2])):
                    raise _Stop(SYNTAX, i)
                k, nxt = (t[i + 1] - 48) * 10 + t[i + 2] - 48, i + 3
            else:
                k, nxt = c - 48, i + 1
            if last < 0 or need_kind in ("(", "."):
                raise _Stop(SYNTAX, i)
            if k in ring:
                other, code, _ = ring.pop(k)
                if other == last or (code and pending and code != pending):
                    raise _Stop(SYNTAX, i)
                if any({a, b} == {other, last} for a, b, _ in bonds):
                    raise _Stop(SYNTAX, i)
                bonds.append((other, last, code or pending))
            else:
                ring[k] = (last, pending, i)
            pending, need, need_kind = 0, -1, ""
            i = nxt
            continue
        elif ch == "(":
            if last < 0 or pending or need_kind in ("(", "."):
                raise _Stop(SYNTAX, i)
            stack.append((last, i))
            need, need_kind = i, "("
            i += 1
            continue
        elif ch == ")":
            if not stack or need >= 0:
                raise _Stop(SYNTAX, i)
            last = stack.pop()[0]
            i += 1
            continue
        elif ch == ".":
            if last < 0 or need >= 0 or stack:
                raise _Stop(SYNTAX, i)
            last, need, need_kind = -1, i, "."
            i += 1
            continue
        else:
            raise _Stop(SYNTAX, i)
        # an atom
        if atom["arom"]:
            flags |= F_AROMATIC
        new = len(atoms)
        atoms.append(atom)
        if last >= 0:
            bonds.append((last, new, pending))
        last, pending, need, need_kind = new, 0, -1, ""
        i = nxt
    ends = [p for p in (unclosed, need if need >= 0 else None, stack[0][1] if stack else None,
                        min((v[2] for v in ring.values()), default=None)) if p is not None]
    if ends:
        raise _Stop(SYNTAX, min(ends))
    return atoms, bonds, flags


def _ring_bond(nbr, a, b):
    """a and b stay connected without their bond"""
    seen, todo = {a}, [j for j in nbr[a] if j != b]
    seen.update(todo)
    while todo:
        j = todo.pop()
        if j == b:
            return True
        for k in nbr[j]:
            if k not in seen:
                seen.add(k)
                todo.append(k)
    return False


def _valence(atom):
    t, q = atom["type"], atom["charge"]
    return {(1, 0): 4, (1, 1): 3, (1, -1): 3, (2, 0): 3, (2, 1): 4, (2, -1): 2, (3, 0): 2, (3, 1): 3}.get((t, q), 0)


def wanting_graph(atoms, order):
    """(wanting atoms, aromatic-bond neighbours among them) of the header's Kekule rule; ``order[a][b]`` is 1..3 or 'a' for an aromatic bond."""
    S = len(atoms)
    sigma = [sum(1 if order[a][b] == "a" else order[a][b] for b in range(S) if order[a][b]) for a in range(S)]
    wants = [a for a in range(S) if atoms[a]["arom"] and _valence(atoms[a]) - sigma[a] - (atoms[a]["h"] or 0) >= 1]
    return wants, {a: [b for b in wants if order[a][b] == "a"] for a in wants}, sigma


def kekule_search(wants, nb, max_nodes):
    """The first perfect matching in the header's order: (status, mate or None, nodes, atom of the last dead end or None)."""
    mate, nodes, fail = {}, 0, None
    levels = []                                 # [atom, cursor, tries]
    while True:
        free = [a for a in wants if a not in mate]
        if not free:
            return OK, mate, nodes, None
        levels.append([free[0], 0, 0])
        while True:
            u, cursor, tries = levels[-1]
            cand = [v for v in nb[u] if v >= cursor and v not in mate]
            if cand:
                if nodes >= max_nodes:
                    return UNDECIDED, None, nodes, None
                nodes += 1
                v = cand[0]
                levels[-1][1], levels[-1][2] = v + 1, tries + 1
                mate[u], mate[v] = v, u
                break
            if tries == 0:
                fail = u
            levels.pop()
            if not levels:
                return KEKULE, None, nodes, fail
            u = levels[-1][0]
            v = mate.pop(u)
            del mate[v]


def read(text, length=None, stride=TEXT_BYTES, max_nodes=4096):
    """One row of ``dsp_read_smiles`` as a dict of FIELDS: ``text`` is ``bytes`` (or an ASCII ``str``), ``length`` its stated length."""
    if isinstance(text, str):
        text = text.encode("latin-1")
    length = len(text) if length is None else length
    out = dict(rec=bytes(RECORD_BYTES), n=0, status=OK, where=-1, string_atoms=0, flags=0, aromatic=0, atom_pos=[-1] * W, nodes=0)
    if length > stride or length < 0:
        return dict(out, status=TOO_LONG)
    if length == 0:
        return dict(out, status=EMPTY)
    t = bytes(text[:length]).ljust(length, b"\0")
    try:
        atoms, bonds, flags = _scan(t)
    except _Stop as s:
        return dict(out, status=s.status, where=s.where)
    S = len(atoms)
    out.update(string_atoms=S, flags=flags)
    if S > W:
        return dict(out, status=TOO_LARGE)
    order = [[0] * S for _ in range(S)]
    nbr = [[] for _ in range(S)]
    for a, b, _ in bonds:
        nbr[a].append(b)
        nbr[b].append(a)
    for a, b, code in bonds:
        if code in (0, SOFT):
            code = "a" if atoms[a]["arom"] and atoms[b]["arom"] and _ring_bond(nbr, a, b) else 1
        order[a][b] = order[b][a] = code
    wants, nb, sigma = wanting_graph(atoms, order)
    status, mate, nodes, fail = kekule_search(wants, nb, max_nodes)
    out["nodes"] = nodes
    if status != OK:
        return dict(out, status=status, where=atoms[fail]["pos"] if status == KEKULE else -1)
    for a in range(S):
        for b in range(S):
            if order[a][b] == "a":
                order[a][b] = 2 if mate.get(a) == b else 1
    hs = []
    for a, atom in enumerate(atoms):
        total = sum(order[a])
        if atom["h"] is not None:
            h = atom["h"]
        elif atom["arom"]:
            h = max(_valence(atom) - sigma[a] - (1 if a in mate else 0), 0)
        else:
            room = [v for v in {1: (4,), 2: (3, 5), 3: (2,), 4: (1,)}[atom["type"]] if v >= total]
            h = room[0] - total if room else 0
        hs.append(h)
    n = S + sum(hs)
    if n > W:
        return dict(out, status=TOO_LARGE)
    rec = np.zeros(RECORD_BYTES, np.uint8)
    bond = np.zeros((W, W), np.uint8)
    bond[:S, :S] = order
    nxt = S
    for a, h in enumerate(hs):
        for _ in range(h):
            bond[a, nxt] = bond[nxt, a] = 1
            nxt += 1
    rec[TYPE:TYPE + S] = [a["type"] for a in atoms]
    rec[FC:FC + S] = np.array([a["charge"] for a in atoms], np.int8).view(np.uint8)
    rec[BOND:BOND + W * W] = bond.reshape(-1)
    return dict(out, rec=rec.tobytes(), n=n, aromatic=sum(1 << a for a in range(S) if atoms[a]["arom"]),
                atom_pos=[a["pos"] for a in atoms] + [-1] * (W - S))


def read_table(texts, lengths=None, stride=TEXT_BYTES, max_nodes=4096):
    return [read(t, None if lengths is None else lengths[k], stride, max_nodes) for k, t in enumerate(texts)]


def molecule(row):
    """The molecule dict (tests/structure_mirror.mol_from_record) of an OK row."""
    rec, n = np.frombuffer(row["rec"], np.uint8), row["n"]
    return dict(pos=np.zeros((n, 3)), type=rec[TYPE:TYPE + n].astype(np.int64), fc=rec[FC:FC + n].view(np.int8).astype(np.int64),
                bond=rec[BOND:BOND + W * W].reshape(W, W)[:n, :n].astype(np.int64))


def pack(strings, stride=TEXT_BYTES):
    """(text [P, stride] u8, length [P] i32) of byte strings: a row longer than the stride keeps its length and is cut."""
    text = np.zeros((len(strings), stride), np.uint8)
    for k, s in enumerate(strings):
        b = s.encode("latin-1") if isinstance(s, str) else bytes(s)
        text[k, :min(len(b), stride)] = np.frombuffer(b[:stride], np.uint8)
    return text, np.array([len(s) for s in strings], np.int32)


# ------------------------------------------------------------------------------------------------------------------ (a) the hand table

def hand_record(symbols, bonds, hydrogens, charges=None):
    """The record a hand-stated molecule must give: string atoms ``symbols`` (lower case = written aromatic), ``bonds`` [(a, b, order)] among
    them, ``hydrogens`` per string atom, ``charges`` {atom: charge}.  Returns (rec bytes, n, aromatic mask)."""
    S = len(symbols)
    rec = np.zeros(RECORD_BYTES, np.uint8)
    bond = np.zeros((W, W), np.uint8)
    for a, b, o in bonds:
        bond[a, b] = bond[b, a] = o
    nxt = S
    for a, h in enumerate(hydrogens):
        for _ in range(h):
            bond[a, nxt] = bond[nxt, a] = 1
            nxt += 1
    rec[TYPE:TYPE + S] = [ELEMENTS[s.upper()] for s in symbols]
    fc = np.zeros(S, np.int8)
    for a, q in (charges or {}).items():
        fc[a] = q
    rec[FC:FC + S] = fc.view(np.uint8)
    rec[BOND:BOND + W * W] = bond.reshape(-1)
    return rec.tobytes(), nxt, sum(1 << a for a, s in enumerate(symbols) if s.islower())


def _chain(k, start=0, order=1):
    return [(start + i, start + i + 1, order) for i in range(k - 1)]


def _cycle(atoms, doubles):
    """The bonds of a ring over ``atoms`` in ring order, order 2 for the pairs in ``doubles``."""
    k = len(atoms)
    pairs = [(atoms[i], atoms[(i + 1) % k]) for i in range(k)]
    return [(a, b, 2 if (a, b) in doubles or (b, a) in doubles else 1) for a, b in pairs]


@functools.lru_cache(maxsize=1)
def hand_table():
    """[(string, symbols, bonds, hydrogens, charges, flags, nodes)]: every molecule, flag word and search length stated by hand."""
    A = F_AROMATIC
    benz = lambda s=0: _cycle([s + i for i in range(6)], {(s, s + 1), (s + 2, s + 3), (s + 4, s + 5)})
    five = _cycle([0, 1, 2, 3, 4], {(0, 4), (1, 2)})
    return [
        # spellings of ethanol and propane
        ("OCC", "OCC", _chain(3), [1, 2, 3], None, 0, 0),
        ("C(O)C", "COC", [(0, 1, 1), (0, 2, 1)], [2, 1, 3], None, 0, 0),
        ("[CH3][CH2][OH]", "CCO", _chain(3), [3, 2, 1], None, 0, 0),
        ("C-C-O", "CCO", _chain(3), [3, 2, 1], None, 0, 0),
        ("C1.O1C", "COC", [(0, 1, 1), (1, 2, 1)], [3, 0, 3], None, 0, 0),
        ("C%10%11.C%10.C%11", "CCC", [(0, 1, 1), (0, 2, 1)], [2, 3, 3], None, 0, 0),
        ("C:C", "CC", [(0, 1, 1)], [3, 3], None, 0, 0),
        ("C(C)(C)C", "CCCC", [(0, 1, 1), (0, 2, 1), (0, 3, 1)], [1, 3, 3, 3], None, 0, 0),
        ("N(C)(C)C", "NCCC", [(0, 1, 1), (0, 2, 1), (0, 3, 1)], [0, 3, 3, 3], None, 0, 0),
        ("C.C", "CC", [], [4, 4], None, 0, 0),
        # charges and brackets
        ("[NH4+]", "N", [], [4], {0: 1}, 0, 0),
        ("C[O-]", "CO", [(0, 1, 1)], [3, 0], {1: -1}, 0, 0),
        ("C[N+](=O)[O-]", "CNOO", [(0, 1, 1), (1, 2, 2), (1, 3, 1)], [3, 0, 0, 0], {1: 1, 3: -1}, 0, 0),
        ("CN(=O)=O", "CNOO", [(0, 1, 1), (1, 2, 2), (1, 3, 2)], [3, 0, 0, 0], None, 0, 0),
        ("[NH3+]CC(=O)[O-]", "NCCOO", [(0, 1, 1), (1, 2, 1), (2, 3, 2), (2, 4, 1)], [3, 2, 0, 0, 0], {0: 1, 4: -1}, 0, 0),
        ("[O--]", "O", [], [0], {0: -2}, 0, 0),
        ("[C+2]", "C", [], [0], {0: 2}, 0, 0),
        ("[N-127]", "N", [], [0], {0: -127}, 0, 0),
        ("[H+]", "H", [], [0], {0: 1}, 0, 0),
        ("[H][H]", "HH", [(0, 1, 1)], [0, 0], None, 0, 0),
        ("[CH3]", "C", [], [3], None, 0, 0),
        ("[C]", "C", [], [0], None, 0, 0),
        ("[2H]O[2H]", "HOH", _chain(3), [0, 0, 0], None, F_ISOTOPE, 0),
        ("[13CH4]", "C", [], [4], None, F_ISOTOPE, 0),
        ("C[C@H](N)O", "CCNO", [(0, 1, 1), (1, 2, 1), (1, 3, 1)], [3, 1, 2, 1], None, F_CHIRAL, 0),
        ("C[C@@H](N)O", "CCNO", [(0, 1, 1), (1, 2, 1), (1, 3, 1)], [3, 1, 2, 1], None, F_CHIRAL, 0),
        ("F/C=C/F", "FCCF", [(0, 1, 1), (1, 2, 2), (2, 3, 1)], [0, 1, 1, 0], None, F_DIRECTION, 0),
        ("C\\C=C\\C", "CCCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1)], [3, 1, 1, 3], None, F_DIRECTION, 0),
        ("[CH3:1][OH:22]", "CO", [(0, 1, 1)], [3, 1], None, F_CLASS, 0),
        # multiple bonds
        ("N#N", "NN", [(0, 1, 3)], [0, 0], None, 0, 0),
        ("O=C=O", "OCO", [(0, 1, 2), (1, 2, 2)], [0, 0, 0], None, 0, 0),
        ("C#N", "CN", [(0, 1, 3)], [1, 0], None, 0, 0),
        # ring closures
        ("C%10CC%10", "CCC", _cycle([0, 1, 2], {}), [2, 2, 2], None, 0, 0),
        ("C1CC1C1CC1", "CCCCCC", _cycle([0, 1, 2], {}) + [(2, 3, 1)] + _cycle([3, 4, 5], {}), [2, 2, 1, 1, 2, 2], None, 0, 0),
        ("C=1CCCCC=1", "CCCCCC", _cycle(list(range(6)), {(5, 0)}), [1, 2, 2, 2, 2, 1], None, 0, 0),
        ("C=1CCCCC1", "CCCCCC", _cycle(list(range(6)), {(5, 0)}), [1, 2, 2, 2, 2, 1], None, 0, 0),
        ("C12CC1C2", "CCCC", [(0, 1, 1), (1, 2, 1), (0, 2, 1), (2, 3, 1), (0, 3, 1)], [1, 2, 1, 2], None, 0, 0),
        ("C0CC0", "CCC", _cycle([0, 1, 2], {}), [2, 2, 2], None, 0, 0),
        ("C1=CC=CC=C1", "CCCCCC", _cycle(list(range(6)), {(0, 1), (2, 3), (4, 5)}), [1] * 6, None, 0, 0),
        # aromatic input: the first matching of the depth-first order, written out
        ("c1ccccc1", "cccccc", benz(), [1] * 6, None, A, 3),
        ("c:1:c:c:c:c:c1", "cccccc", benz(), [1] * 6, None, A, 3),
        ("c1ccncc1", "cccncc", benz(), [1, 1, 1, 0, 1, 1], None, A, 3),
        ("c1cc[nH]c1", "cccnc", five, [1] * 5, None, A, 3),
        ("c1ccoc1", "cccoc", five, [1, 1, 1, 0, 1], None, A, 3),
        ("c1cc[cH-]c1", "ccccc", five, [1] * 5, {3: -1}, A, 3),
        ("[nH]1cccc1", "ncccc", _cycle([0, 1, 2, 3, 4], {(1, 2), (3, 4)}), [1] * 5, None, A, 2),
        ("c1cnc[nH]1", "ccncn", _cycle([0, 1, 2, 3, 4], {(0, 1), (2, 3)}), [1, 1, 0, 1, 1], None, A, 2),
        ("O=c1cccc[nH]1", "Occcccn", [(0, 1, 2)] + _cycle([1, 2, 3, 4, 5, 6], {(2, 3), (4, 5)}), [0, 0, 1, 1, 1, 1, 1], None, A, 2),
        ("[O-][n+]1ccccc1", "Onccccc", [(0, 1, 1)] + _cycle([1, 2, 3, 4, 5, 6], {(1, 2), (3, 4), (5, 6)}), [0, 0, 1, 1, 1, 1, 1],
         {0: -1, 1: 1}, A, 3),
        ("c1ccccc1O", "ccccccO", benz() + [(5, 6, 1)], [1, 1, 1, 1, 1, 0, 1], None, A, 3),
        ("c1ccc2ccccc2c1", "c" * 10, [(0, 1, 2), (1, 2, 1), (2, 3, 2), (3, 4, 1), (4, 5, 2), (5, 6, 1), (6, 7, 2), (7, 8, 1), (3, 8, 1), (8, 9, 2),
                                      (0, 9, 1)], [1, 1, 1, 0, 1, 1, 1, 1, 0, 1], None, A, 5),
        ("c1ccc2cccc2cc1", "c" * 10, [(0, 1, 2), (1, 2, 1), (2, 3, 2), (3, 4, 1), (4, 5, 2), (5, 6, 1), (6, 7, 2), (3, 7, 1), (7, 8, 1), (8, 9, 2),
                                      (0, 9, 1)], [1, 1, 1, 0, 1, 1, 1, 0, 1, 1], None, A, 5),
        ("c1ccccc1c1ccccc1", "c" * 12, benz() + [(5, 6, 1)] + benz(6), [1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1], None, A, 6),
        ("c1ccc(cc1)-c1ccccc1", "c" * 12, benz() + [(3, 6, 1)] + benz(6), [1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1], None, A, 6),
        # 2-methylpyridine: the drawing depends on where the string starts; each is the first matching of its string
        ("Cc1ccccn1", "Ccccccn", [(0, 1, 1)] + _cycle([1, 2, 3, 4, 5, 6], {(1, 2), (3, 4), (5, 6)}), [3, 0, 1, 1, 1, 1, 0], None, A, 3),
        ("n1ccccc1C", "ncccccC", _cycle([0, 1, 2, 3, 4, 5], {(0, 1), (2, 3), (4, 5)}) + [(5, 6, 1)], [0, 1, 1, 1, 1, 0, 3], None, A, 3),
    ]


def hand_rows():
    """The rows the hand table states, as ``read`` returns them (``atom_pos`` apart, which the strings give: see ``symbol_positions``)."""
    rows = []
    for text, symbols, bonds, hydrogens, charges, flags, nodes in hand_table():
        rec, n, aromatic = hand_record(symbols, bonds, hydrogens, charges)
        rows.append(dict(rec=rec, n=n, status=OK, where=-1, string_atoms=len(symbols), flags=flags, aromatic=aromatic,
                         atom_pos=symbol_positions(text, symbols), nodes=nodes))
    return rows


def symbol_positions(text, symbols):
    """Byte offsets of the atoms' symbols by a plain left-to-right search for each symbol in turn (no tokenizer): skips digits of isotopes,
    the H of a hydrogen count (which follows its atom's symbol inside the same bracket) and bond, ring and branch characters."""
    out, at, inside, seen = [], 0, False, False
    for s in symbols:
        while True:
            c = text[at]
            if c == "[":
                inside, seen = True, False
            elif c == "]":
                inside = False
            elif c == s and (not inside or not seen) and c.isalpha():
                seen = True
                out.append(at)
                at += 1
                break
            at += 1
    return out + [-1] * (W - len(out))


# ------------------------------------------------------------------------------------------------------------------ (b) the error table

@functools.lru_cache(maxsize=1)
def error_table():
    """[(string, status, where, string_atoms, nodes)], every entry stated by hand."""
    S, E = SYNTAX, ELEMENT
    rows = [
        ("C(", S, 1), ("C)", S, 1), ("()", S, 0), ("C((C))", S, 2), ("C==C", S, 2), ("C1CC", S, 1), ("C11", S, 2), ("C12CCC12", S, 7),
        ("C=1CCC-1", S, 7), ("[C", S, 0), ("[]", S, 1), ("[CH", S, 0), ("C%1", S, 1), ("C$C", S, 1), ("Hc", S, 0),
        ("CS", E, 1), ("CCl", E, 1), ("[Na+]", E, 1), ("C*", E, 1), ("CBr", E, 1), ("[Cl-]", E, 1), ("Cb", E, 1), ("[se]", E, 1), ("[Xe]", E, 1),
        ("CI", E, 1), ("CP", E, 1), ("[*]", E, 1), ("[Co]", E, 1), ("[Hg]", E, 1),
        ("=C", S, 0), ("C=", S, 1), ("C#", S, 1), ("C.", S, 1), (".C", S, 0), ("C..C", S, 2), ("C(C", S, 1), ("C()", S, 2), ("C(=)C", S, 3),
        ("C=(C)C", S, 2), ("1CC1", S, 0), ("C(1CC1)", S, 2), ("[C+++]", S, 4), ("[C+128]", S, 2), ("[C+1000]", S, 6), ("[CH3", S, 0),
        ("[C@TH1]", S, 3), ("[C:]", S, 3), ("C C", S, 1), ("C1CC2", S, 1), ("C(C.C)", S, 3), ("C[", S, 1), ("C%", S, 1), ("C%a1", S, 1),
        ("[12", S, 0), ("[1]", S, 2), ("[CH2H]", S, 4), ("[x]", S, 1), ("[C]]", S, 3), ("C-=C", S, 2), ("C1CC(", S, 1), ("C\xffC", S, 1),
        ("CC(C)1", S, 5), ("C(C)=", S, 4), ("C.(C)", S, 2), ("C\x00", S, 1), ("[C++2]", S, 4), ("[HC]", S, 2),
    ]
    out = [(t, st, w, 0, 0) for t, st, w in rows]
    out += [("c1ccnc1", KEKULE, 4, 5, 4), ("cC", KEKULE, 0, 2, 0), ("cc", KEKULE, 0, 2, 0),
            ("CCCCCCCCCC", TOO_LARGE, -1, 10, 0), ("CCCCCCCCCO", TOO_LARGE, -1, 10, 0), (".".join(["[C]"] * 30), TOO_LARGE, -1, 30, 0),
            ("", EMPTY, -1, 0, 0)]
    return out


def limit_pairs():
    """[(29-atom string, 30-atom string)] side by side: the first reads OK with n = 29, the second is TOO_LARGE."""
    return [("CCCCCCCCC", "CCCCCCCCCO"), (".".join(["[C]"] * 29), ".".join(["[C]"] * 30)), ("c1ccccc1CCCCCN", "c1ccccc1CCCCCC"),
            ("[CH4].[CH4].[CH4].[CH4].[CH4].[H][H].[H][H]", "[CH4].[CH4].[CH4].[CH4].[CH4].[H][H].[H][H].[H]")]


# ------------------------------------------------------------------------------------------------------------------ (c) the generator

_VALENCE = {"C": 4, "N": 3, "O": 2, "F": 1}
# bracket atoms: (text, bonds it may take, hydrogens it brings)
_BRACKETS = (("[O-]", 1, 0), ("[NH3+]", 1, 3), ("[NH2+]", 2, 2), ("[N+]", 4, 0), ("[CH2]", 2, 2), ("[CH]", 3, 1), ("[C@H]", 3, 1), ("[C@@H]", 3, 1),
             ("[13CH3]", 1, 3), ("[OH]", 1, 1), ("[C-]", 3, 0), ("[CH3:7]", 1, 3), ("[2H]", 1, 0), ("[NH+]", 3, 1), ("[OH+]", 2, 1))
# aromatic rings: the atoms in ring order, (text, substituents it may take, hydrogens without one)
_RINGS = (("c", "c", "c", "c", "c", "c"), ("c", "c", "n", "c", "c", "c"), ("c", "c", "[nH]", "c", "c"), ("c", "o", "c", "c", "c"),
          ("n", "c", "c", "c", "c", "c"), ("[nH]", "c", "c", "c", "c"), ("c", "c", "c", "n", "c", "n"))


class _Builder:
    """A molecule as a tree of atoms with ring-closure edges; ``total`` = atoms of the string + hydrogens they carry."""

    def __init__(self, rng):
        self.rng = rng
        self.text, self.free, self.kind, self.fixed_h = [], [], [], []      # kind: 'bare', 'bracket', 'arom'
        self.parent, self.order, self.children, self.closures = [], [], [], []
        self.roots = []

    def total(self):
        t = len(self.text)
        for a in range(len(self.text)):
            if self.kind[a] == "bare":
                t += self.free[a]                    # what is left of the valence is hydrogens
            elif self.kind[a] == "bracket":
                t += self.fixed_h[a]
            else:
                t += self.fixed_h[a] if self.text[a] == "[nH]" else (self.free[a] if self.text[a] == "c" else 0)
        return t

    def add(self, text, kind, free, fixed_h, parent, order):
        a = len(self.text)
        self.text.append(text); self.kind.append(kind); self.free.append(free); self.fixed_h.append(fixed_h)
        self.parent.append(parent); self.order.append(order); self.children.append([])
        if parent is None:
            self.roots.append(a)
        else:
            self.children[parent].append(a)
            self.free[parent] -= order
            self.free[a] -= order
        return a

    def snapshot(self):
        return ([list(x) for x in (self.text, self.free, self.kind, self.fixed_h, self.parent, self.order)], [list(c) for c in self.children],
                list(self.closures), list(self.roots))

    def restore(self, s):
        (self.text, self.free, self.kind, self.fixed_h, self.parent, self.order), self.children, self.closures, self.roots = s

    def grow(self):
        """One random step; undone when it would pass 29 atoms.  Returns False when nothing was added."""
        rng, s = self.rng, self.snapshot()
        open_ = [a for a in range(len(self.text)) if self.free[a] >= 1]
        kind = rng.integers(0, 10)
        if not self.text or kind == 0:
            parent = None                            # a new component
        elif not open_:
            return False
        else:
            parent = int(open_[rng.integers(len(open_))])
        if kind <= 1 and len(open_) >= 2 and parent is not None:                # a ring closure between two bare atoms
            a, b = (int(x) for x in rng.choice(open_, 2, replace=False))
            bonded = self.parent[a] == b or self.parent[b] == a or any({a, b} == {x, y} for x, y, _ in self.closures)
            if self.kind[a] == "bare" and self.kind[b] == "bare" and not bonded:
                o = 2 if min(self.free[a], self.free[b]) >= 2 and rng.integers(4) == 0 else 1
                self.closures.append((min(a, b), max(a, b), o))
                self.free[a] -= o
                self.free[b] -= o
                return True
            return False
        if kind <= 3:                                                           # an aromatic ring
            ring = _RINGS[rng.integers(len(_RINGS))]
            k0 = int(rng.integers(len(ring)))
            ring = ring[k0:] + ring[:k0]
            if parent is not None and ring[0] != "c":
                ring = _RINGS[0]                     # only a c takes the bond to the parent
            first = prev = None
            for x in ring:
                free = {"c": 3, "n": 2, "o": 2, "[nH]": 2}[x]                   # ring bonds count 1 each; a c keeps one place
                a = self.add(x, "arom", free, 1 if x == "[nH]" else 0, parent if prev is None else prev, 1 if prev is not None or parent is not None else 0)
                first = a if first is None else first
                prev = a
            self.closures.append((first, prev, 0))
            self.free[first] -= 1
            self.free[prev] -= 1
        elif kind <= 5:                                                         # a bracket atom
            text, bonds, h = _BRACKETS[rng.integers(len(_BRACKETS))]
            self.add(text, "bracket", bonds, h, parent, 1)
        else:                                                                   # a bare atom, by a bond of order 1..3
            sym = "CCCNOF"[rng.integers(6)]
            room = 3 if parent is None else min(3, self.free[parent], _VALENCE[sym])
            o = 1 if parent is None or self.kind[parent] != "bare" or rng.integers(3) else int(rng.integers(1, room + 1))
            self.add(sym, "bare", _VALENCE[sym], 0, parent, o if parent is not None else 0)
        if min(self.free) < 0 or self.total() > W:
            self.restore(s)
            return False
        return True

    def write(self):
        rng = self.rng
        sym = {0: "", 1: "", 2: "=", 3: "#"}
        numbers = {}                                 # closure index -> number
        in_use = set()
        out = []

        def number(k):
            return str(k) if k < 10 and rng.integers(8) else "%%%02d" % k

        def emit(a):
            out.append(self.text[a])
            for c, (x, y, o) in enumerate(self.closures):
                if y == a and c in numbers:          # close (the atom visited second)
                    k = numbers.pop(c)
                    out.append((sym[o] if o >= 2 and rng.integers(2) else "") + number(k))
                    in_use.discard(k)
                elif x == a or y == a:
                    pool = [k for k in range(0, 100) if k not in in_use]
                    k = pool[0] if rng.integers(4) else int(pool[rng.integers(len(pool))])
                    numbers[c] = k
                    in_use.add(k)
                    out.append((sym[o] if o >= 2 else "") + number(k))
            kids = self.children[a]
            for b in kids:
                o = self.order[b]
                dash = "-/\\"[rng.integers(3)] if o == 1 and rng.integers(10) == 0 and not (self.kind[a] == "arom" and self.kind[b] == "arom") else ""
                branch = b != kids[-1] or rng.integers(10) == 0
                out.append(("(" if branch else "") + sym[o] + dash)
                emit(b)
                if branch:
                    out.append(")")
        for r in self.roots:
            if out:
                out.append(".")
            emit(r)
        return "".join(out)


def _visit_order_ok(builder):
    """closures are written at the atom visited first; ``write`` needs x visited before y: true when x < y in depth-first preorder, which holds
    because atoms are numbered in creation order only per subtree - so renumber the closures by the preorder here."""
    order, seen = {}, []

    def walk(a):
        order[a] = len(seen)
        seen.append(a)
        for b in builder.children[a]:
            walk(b)
    for r in builder.roots:
        walk(r)
    builder.closures = [(x, y, o) if order[x] < order[y] else (y, x, o) for x, y, o in builder.closures]


@functools.lru_cache(maxsize=4)
def generated(count=2000, seed=20261021):
    """``count`` valid strings (a tuple): random trees with ring closures, charges, brackets, isotopes, classes and lower-case benzene,
    pyridine, pyrimidine, pyrrole and furan rings; never more than 29 atoms with the hydrogens, so every one reads OK."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        b = _Builder(rng)
        for _ in range(int(rng.integers(1, 14))):
            b.grow()
        if not b.text:
            continue
        _visit_order_ok(b)
        s = b.write()
        if len(s) <= TEXT_BYTES:
            out.append(s)
    return tuple(out)


_EDIT_ALPHABET = "CCNOFcno[]()=#-:/\\.%0123456789+@HSlBr*$ "


@functools.lru_cache(maxsize=4)
def edited(count=2000, seed=20261022):
    """One random single-byte edit (replace, insert, delete) of each generated string."""
    rng = np.random.default_rng(seed)
    out = []
    for s in generated(count):
        at, ch = int(rng.integers(len(s) + 1)), _EDIT_ALPHABET[rng.integers(len(_EDIT_ALPHABET))]
        kind = rng.integers(3)
        if kind == 0 and at < len(s):
            s = s[:at] + ch + s[at + 1:]
        elif kind == 1:
            s = s[:at] + ch + s[at:]
        else:
            at = min(at, len(s) - 1)
            s = s[:at] + s[at + 1:]
        out.append(s)
    return tuple(out)


EDIT_STRIDE, EDIT_MAX_NODES = 40, 3     # the edited set is read at a short stride and a small budget, so TOO_LONG and UNDECIDED occur in it
