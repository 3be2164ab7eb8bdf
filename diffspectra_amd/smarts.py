"""A SMARTS subset compiled to the pattern words of ``include/diffspectra_substructure.h`` (``dsq_match_records``): plain host code, no RDKit.

What is accepted
    Atoms    bare ``*``, ``a``, ``A`` and the organic-subset symbols (``B C N O P S F Cl Br I``, lower case ``b c n o p s`` = aromatic); bracket
             atoms of ``;``-separated clauses.  A clause is one alternative or several ``,``-alternatives; an alternative is a juxtaposition or
             ``&`` of primitives, each optionally negated with ``!`` (the complement within the primitive's property).  A clause with several
             alternatives is accepted only when every alternative constrains the same single property (``H2,H3``; ``F,Cl,Br,I``).
             Primitives: ``*``, ``a``, ``A``, ``#n``, element symbols, ``H<n>`` (total hydrogens; ``H`` = ``H1``; a hydrogen ATOM is ``#1``),
             ``X<n>``, ``D<n>`` (``X`` = ``X1``, ``D`` = ``D1``), ``R`` (ring atom), ``R0`` (chain atom), ``+0``, ``+``, ``+1``, ``-``, ``-1``.  The counts
             saturate as the kernel's do: ``H4``, ``X4`` and ``D4`` mean "4 or more".  An element outside H, C, N, O, F maps to the empty set:
             the pattern is legal and never matches.
    Bonds    ``- = # : ~ @`` combined with ``!``, ``&``, ``,`` and ``;`` (precedence ``!`` > ``&`` > ``,`` > ``;``): a subset of the eight classes
             {single, double, triple, aromatic} x {chain, ring}.  An omitted bond is "single or aromatic".
    Shape    chains, branches, ring-closure digits 1-9; the closure's bond may be written at either end, and at both only when equal.

Everything else raises ``ValueError`` naming the construct: recursive ``$()``, dots, atom maps, chirality, isotopes, ``r``, ``x``, ``v``, ``h``, ``R<n>``
with n > 0, charges beyond +-1, more than 14 atoms, more than 2 closures, a ``,``-clause over mixed properties."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import abi

_K = abi.SUBSTRUCTURE.consts
WORDS, MAX_ATOMS, MAX_CLOSURES = _K["DSQ_PATTERN_WORDS"], _K["DSQ_MAX_PATTERN_ATOMS"], _K["DSQ_MAX_CLOSURES"]
WORD_ATOM, WORD_LINK, WORD_CLOSURE = _K["DSQ_WORD_ATOM"], _K["DSQ_WORD_LINK"], _K["DSQ_WORD_CLOSURE"]
# property -> (first bit, number of bits)
FIELDS = {"element": (_K["DSQ_BIT_ELEMENT"], 10), "Ht": (_K["DSQ_BIT_HT"], 5), "X": (_K["DSQ_BIT_X"], 5), "D": (_K["DSQ_BIT_D"], 5),
          "ring": (_K["DSQ_BIT_RING"], 2), "charge": (_K["DSQ_BIT_CHARGE"], 3)}
ELEMENTS = "HCNOF"                                                             # the record's atom types 0..4
ATOMIC_NUMBER = {1: 0, 6: 1, 7: 2, 8: 3, 9: 4}
SINGLE, DOUBLE, TRIPLE, AROMATIC, RING, ANY_BOND = 0x11, 0x22, 0x44, 0x88, 0xF0, 0xFF          # bond-class sets: bit kind + 4 * ring
DEFAULT_BOND = SINGLE | AROMATIC
_TWO_LETTER = ("Cl", "Br", "Si", "Se", "As", "Na", "Li", "Mg", "Al", "Ca", "Fe", "Zn", "Cu", "Sn", "Te", "Ge")
_ONE_LETTER = "BCNOFPSIK"
_AROMATIC_LETTER = "bcnops"
_BOND_CHARS = "-=#:~@!&,;"


def _full(prop):
    return (1 << FIELDS[prop][1]) - 1


def _element_set(symbol: str, aromatic: bool) -> int:
    """The element field of a symbol: aliphatic or aromatic bit of H, C, N, O, F; empty for every other element."""
    if symbol.upper() in ELEMENTS and len(symbol) == 1:
        return 1 << (2 * ELEMENTS.index(symbol.upper()) + int(aromatic))
    return 0


def _number(text: str, i: int) -> Tuple[int, int]:
    """(value or None, next index) of the digits at ``text[i:]``."""
    j = i
    while j < len(text) and text[j].isdigit():
        j += 1
    return (int(text[i:j]) if j > i else None), j


def _primitive(text: str, i: int, whole: str) -> Tuple[str, int, int]:
    """One atom primitive at ``text[i:]`` -> (property, allowed set within it, next index); ``*`` returns property None."""
    c = text[i]
    if c == "*":
        return None, 0, i + 1
    if c == "$":
        raise ValueError(f"{whole!r}: recursive SMARTS $() is not supported")
    if c == "@":
        raise ValueError(f"{whole!r}: chirality (@) is not supported")
    if c == ":":
        raise ValueError(f"{whole!r}: atom maps (:n) are not supported")
    if c.isdigit():
        raise ValueError(f"{whole!r}: isotopes are not supported")
    if c == "#":
        n, j = _number(text, i + 1)
        if n is None:
            raise ValueError(f"{whole!r}: '#' needs an atomic number")
        return "element", (3 << (2 * ATOMIC_NUMBER[n])) if n in ATOMIC_NUMBER else 0, j
    if text[i:i + 2] in _TWO_LETTER:
        return "element", 0, i + 2
    if c == "a":
        return "element", 0x2AA, i + 1
    if c == "A":
        return "element", 0x155, i + 1
    if c == "H":
        n, j = _number(text, i + 1)
        n = 1 if n is None else n
        if n > 4:
            raise ValueError(f"{whole!r}: H{n}: hydrogen counts go up to 4 (H4 = 4 or more)")
        return "Ht", 1 << n, j
    if c in "XD":
        n, j = _number(text, i + 1)
        n = 1 if n is None else n
        if n > 4:
            raise ValueError(f"{whole!r}: {c}{n}: counts go up to 4 ({c}4 = 4 or more)")
        return c, 1 << n, j
    if c == "R":
        n, j = _number(text, i + 1)
        if n is not None and n > 0:
            raise ValueError(f"{whole!r}: R{n} (a ring count) is not supported, only R and R0")
        return "ring", 1 if n == 0 else 2, j
    if c in "rxvh^":
        raise ValueError(f"{whole!r}: the primitive '{c}' is not supported")
    if c in "+-":
        n, j = _number(text, i + 1)
        if n is None and text[i + 1:i + 2] == c:
            raise ValueError(f"{whole!r}: charges beyond +1 / -1 are not supported")
        n = 1 if n is None else n
        if n > 1:
            raise ValueError(f"{whole!r}: charges beyond +1 / -1 are not supported")
        return "charge", 1 << (1 + (n if c == "+" else -n)), j
    if c in _ONE_LETTER:
        return "element", _element_set(c, False), i + 1
    if c in _AROMATIC_LETTER:
        return "element", _element_set(c, True), i + 1
    raise ValueError(f"{whole!r}: cannot read {text[i:]!r} in a bracket atom")


def _alternative(text: str, whole: str) -> Dict[str, int]:
    """A juxtaposition / ``&`` of primitives -> {property: allowed set}."""
    if not text:
        raise ValueError(f"{whole!r}: an empty atom expression")
    out: Dict[str, int] = {}
    i = 0
    while i < len(text):
        if text[i] == "&":
            i += 1
            continue
        negate = text[i] == "!"
        if negate:
            i += 1
            if i >= len(text):
                raise ValueError(f"{whole!r}: '!' without a primitive")
        prop, allowed, i = _primitive(text, i, whole)
        if prop is None:
            if negate:
                raise ValueError(f"{whole!r}: '!*' is not supported")
            continue
        if negate:
            allowed = _full(prop) & ~allowed
        out[prop] = out.get(prop, _full(prop)) & allowed
    return out


def _bracket_atom(text: str, whole: str) -> int:
    sets = {prop: _full(prop) for prop in FIELDS}
    for clause in text.split(";"):
        alternatives = [_alternative(a, whole) for a in clause.split(",")]
        if len(alternatives) == 1:
            merged = alternatives[0]
        else:
            props = {p for a in alternatives for p in a}
            if len(props) != 1 or any(len(a) != 1 for a in alternatives):
                raise ValueError(f"{whole!r}: the clause {clause!r} mixes properties across its ','-alternatives; only one property per clause")
            prop = props.pop()
            merged = {prop: 0}
            for a in alternatives:
                merged[prop] |= a[prop]
        for prop, allowed in merged.items():
            sets[prop] &= allowed
    return sum(sets[prop] << FIELDS[prop][0] for prop in FIELDS)


def _bare_atom(symbol: str) -> int:
    sets = {prop: _full(prop) for prop in FIELDS}
    if symbol == "a":
        sets["element"] = 0x2AA
    elif symbol == "A":
        sets["element"] = 0x155
    elif symbol != "*":
        sets["element"] = _element_set(symbol, symbol.islower())
    return sum(sets[prop] << FIELDS[prop][0] for prop in FIELDS)


def _bond_set(text: str, whole: str) -> int:
    """A bond expression -> a set of the eight classes; '' is the omitted bond."""
    if not text:
        return DEFAULT_BOND
    basic = {"-": SINGLE, "=": DOUBLE, "#": TRIPLE, ":": AROMATIC, "~": ANY_BOND, "@": RING}
    result = ANY_BOND
    for low in text.split(";"):
        union = 0
        for alt in low.split(","):
            if not alt.replace("&", ""):
                raise ValueError(f"{whole!r}: an empty bond expression in {text!r}")
            part, negate = ANY_BOND, False
            for c in alt:
                if c == "&":
                    continue
                if c == "!":
                    negate = not negate
                    continue
                part &= (ANY_BOND & ~basic[c]) if negate else basic[c]
                negate = False
            if negate:
                raise ValueError(f"{whole!r}: '!' without a bond in {text!r}")
            union |= part
        result &= union
    return result


def parse(text: str):
    """``text`` -> (atom words [A], links [(parent, bond set)] for atoms 1.., closures [(a, b, bond set)])."""
    if not isinstance(text, str):
        raise TypeError(f"a pattern is a str, got {type(text).__name__}")
    atoms: List[int] = []
    links: List[Tuple[int, int]] = []
    closures: List[Tuple[int, int, int]] = []
    open_rings: Dict[int, Tuple[int, str]] = {}
    stack: List[int] = []
    prev, bond, i = None, None, 0                                             # bond: the expression written since the last atom, None = none

    def add(word):
        nonlocal prev, bond
        if len(atoms) == MAX_ATOMS:
            raise ValueError(f"{text!r}: more than {MAX_ATOMS} atoms")
        if prev is None:
            if atoms:
                raise ValueError(f"{text!r}: an atom without a bond to what is before it")
            if bond is not None:
                raise ValueError(f"{text!r}: a bond before the first atom")
        else:
            links.append((prev, _bond_set(bond or "", text)))
        atoms.append(word)
        prev, bond = len(atoms) - 1, None

    while i < len(text):
        c = text[i]
        if c == "[":
            j = text.find("]", i)
            if j < 0:
                raise ValueError(f"{text!r}: '[' without ']'")
            add(_bracket_atom(text[i + 1:j], text))
            i = j + 1
        elif c in _BOND_CHARS:
            j = i
            while j < len(text) and text[j] in _BOND_CHARS:
                j += 1
            if bond is not None or prev is None:
                raise ValueError(f"{text!r}: a bond with nothing to bond at position {i}")
            bond, i = text[i:j], j
        elif c == "(":
            if prev is None or bond is not None:
                raise ValueError(f"{text!r}: '(' at position {i} does not follow an atom")
            stack.append(prev)
            i += 1
        elif c == ")":
            if not stack or bond is not None:
                raise ValueError(f"{text!r}: ')' at position {i} closes nothing")
            prev = stack.pop()
            i += 1
        elif c.isdigit():
            if prev is None or c == "0":
                raise ValueError(f"{text!r}: ring-closure digit '{c}' at position {i}")
            d = int(c)
            if d in open_rings:
                a, first = open_rings.pop(d)
                if a == prev:
                    raise ValueError(f"{text!r}: ring closure {d} joins an atom to itself")
                if first is not None and bond is not None and _bond_set(first, text) != _bond_set(bond, text):
                    raise ValueError(f"{text!r}: ring closure {d} is written with two different bonds, {first!r} and {bond!r}")
                if len(closures) == MAX_CLOSURES:
                    raise ValueError(f"{text!r}: more than {MAX_CLOSURES} ring closures")
                closures.append((a, prev, _bond_set(first if first is not None else (bond or ""), text)))
            else:
                open_rings[d] = (prev, bond)
            bond = None
            i += 1
        elif c == ".":
            raise ValueError(f"{text!r}: dots (disconnected patterns) are not supported")
        elif c == "%":
            raise ValueError(f"{text!r}: ring closures above 9 (%nn) are not supported")
        elif c in "/\\":
            raise ValueError(f"{text!r}: directional bonds (chirality) are not supported")
        elif c == "$":
            raise ValueError(f"{text!r}: recursive SMARTS $() is not supported")
        elif text[i:i + 2] in ("Cl", "Br"):
            add(_bare_atom(text[i:i + 2]))
            i += 2
        elif c in "*aA" or c in "BCNOPSFI" or c in _AROMATIC_LETTER:
            add(_bare_atom(c))
            i += 1
        else:
            raise ValueError(f"{text!r}: cannot read {text[i:]!r}")
    if not atoms:
        raise ValueError(f"{text!r}: a pattern needs an atom")
    if bond is not None or stack or open_rings:
        raise ValueError(f"{text!r}: an unfinished bond, branch or ring closure")
    return atoms, links, closures


def pack(atoms: Sequence[int], links: Sequence[Tuple[int, int]], closures: Sequence[Tuple[int, int, int]]) -> np.ndarray:
    """The 32 words of the header from parsed parts."""
    words = np.zeros(WORDS, np.int64)
    words[0] = len(atoms) | (len(closures) << 8)
    for k, w in enumerate(atoms):
        words[WORD_ATOM + k] = w
    for k, (parent, bonds) in enumerate(links, start=1):
        words[WORD_LINK + k] = parent | (bonds << 8)
    for c, (a, b, bonds) in enumerate(closures):
        words[WORD_CLOSURE + c] = a | (b << 8) | (bonds << 16)
    return words.astype(np.int32)


def compile_pattern(text: str) -> np.ndarray:
    """One pattern text -> ``int32 [32]``."""
    return pack(*parse(text))


def compile_patterns(texts: Sequence[str]) -> np.ndarray:
    """Pattern texts -> ``int32 [K, 32]``, a row per text in order."""
    if isinstance(texts, str):
        raise TypeError("compile_patterns takes a sequence of pattern texts; compile_pattern takes one")
    rows = [compile_pattern(t) for t in texts]
    return np.stack(rows) if rows else np.zeros((0, WORDS), np.int32)
