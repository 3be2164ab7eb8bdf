"""The 166 MACCS keys as data for the substructure matcher (``include/diffspectra_substructure.h``, ``smarts.py``): ``MACCS_KEYS[key - 1] = (name,
alternatives, threshold)``.  ``alternatives`` is a list of pattern texts, or ``None`` for a key that is constant 0 here (its element or property
cannot occur among H, C, N, O, F) and for the two keys computed from per-record outputs (``SPECIAL``).  A key is set iff its number of matches
exceeds ``threshold``: for one pattern the number of matches is the kernel's ``count`` (distinct atom sets, RDKit's uniquified matches); for a key
that RDKit writes as one recursive atom ``[$(...),$(...)]`` the matches are ATOMS - the popcount of the OR of the alternatives' ``anchors``.

The table restates RDKit's ``MACCSkeys.smartsPatts`` AS REMEMBERED: RDKit cannot be run where this project runs, so parity with RDKit is
UNPINNED.  A misremembered key is a one-line fix here, never a kernel change.  Stated deviations: the patterns run on the hydrogen-folded
graph; aromaticity is the project's rule (``include/diffspectra_groups.h``); only applied charges count for key 49; ring keys are SMARTS
cycles, as in RDKit, not SSSR rings."""
from __future__ import annotations

NUM_KEYS = 166
CONSTANT_ZERO = frozenset([1, 2, 3, 4, 5, 6, 7, 9, 10, 12, 14, 18, 20, 27, 29, 32, 33, 35, 36, 39, 40, 44, 46, 47, 51, 55, 58, 59, 60, 61, 64, 67,
                           73, 81, 88, 103])
SPECIAL = {125: "aromatic_rings > 1", 166: "fragments > 1"}

_Q, _QH = "[!#6;!#1]", "[!#6;!#1;!H0]"
_X = "[F,Cl,Br,I]"


def _cycle(size):
    return "[R]@1" + "@[R]" * (size - 1) + "1"


# key: (pattern, threshold)
_SINGLE = {
    8: (_Q + "1~*~*~*~1", 0), 11: ("*1~*~*~*~1", 0), 13: ("[#8]~[#7](~[#6])~[#6]", 0), 15: ("[#8]~[#6](~[#8])~[#8]", 0),
    16: (_Q + "1~*~*~1", 0), 17: ("[#6]#[#6]", 0), 19: ("*1~*~*~*~*~*~*~1", 0), 21: ("[#6]=[#6](~" + _Q + ")~" + _Q, 0),
    22: ("*1~*~*~1", 0), 23: ("[#7]~[#6](~[#8])~[#8]", 0), 24: ("[#7]-[#8]", 0), 25: ("[#7]~[#6](~[#7])~[#7]", 0),
    26: ("[#6]=;@[#6](@*)@*", 0), 28: (_Q + "~[CH2]~" + _Q, 0), 30: ("[#6]~" + _Q + "(~[#6])(~[#6])~*", 0),
    31: (_Q + "~" + _X, 0), 34: ("[CH2]=*", 0), 37: ("[#7]~[#6](~[#8])~[#7]", 0), 38: ("[#7]~[#6](~[#6])~[#7]", 0),
    41: ("[#6]#[#7]", 0), 42: ("F", 0), 43: (_QH + "~*~" + _QH, 0),
    45: ("[#6]=[#6]~[#7]", 0), 48: ("[#8]~" + _Q + "(~[#8])(~[#8])", 0), 49: ("[!+0]", 0),
    50: ("[#6]=[#6](~[#6])~[#6]", 0), 52: ("[#7]~[#7]", 0), 53: (_QH + "~*~*~*~" + _QH, 0),
    54: (_QH + "~*~*~" + _QH, 0), 56: ("[#8]~[#7](~[#8])~[#6]", 0), 57: ("[#8R]", 0),
    62: ("*@*!@*@*", 0), 63: ("[#7]=[#8]", 0), 65: ("c:n", 0), 66: ("[#6]~[#6](~[#6])(~[#6])~*", 0),
    68: (_QH + "~" + _QH, 0), 69: (_Q + "~" + _QH, 0), 70: (_Q + "~[#7]~" + _Q, 0),
    71: ("[#7]~[#8]", 0), 72: ("[#8]~*~*~[#8]", 0), 74: ("[CH3]~*~[CH3]", 0), 75: ("*!@[#7]@*", 0),
    76: ("[#6]=[#6](~*)~*", 0), 77: ("[#7]~*~[#7]", 0), 78: ("[#6]=[#7]", 0), 79: ("[#7]~*~*~[#7]", 0),
    80: ("[#7]~*~*~*~[#7]", 0), 82: ("*~[CH2]~" + _QH, 0), 83: (_Q + "1~*~*~*~*~1", 0), 84: ("[NH2]", 0),
    85: ("[#6]~[#7](~[#6])~[#6]", 0), 86: ("[C;H2,H3]" + _Q + "[C;H2,H3]", 0), 87: (_X + "!@*@*", 0),
    89: ("[#8]~*~*~*~[#8]", 0), 92: ("[#8]~[#6](~[#7])~[#6]", 0), 93: (_Q + "~[CH3]", 0), 94: (_Q + "~[#7]", 0),
    95: ("[#7]~*~*~[#8]", 0), 96: ("*1~*~*~*~*~1", 0), 97: ("[#7]~*~*~*~[#8]", 0), 98: (_Q + "1~*~*~*~*~*~1", 0),
    99: ("[#6]=[#6]", 0), 100: ("*~[CH2]~[#7]", 0), 102: (_Q + "~[#8]", 0), 104: (_QH + "~*~[CH2]~*", 0),
    105: ("*@*(@*)@*", 0), 106: (_Q + "~*(~" + _Q + ")~" + _Q, 0), 107: (_X + "~*(~*)~*", 0),
    108: ("[CH3]~*~*~*~[CH2]~*", 0), 109: ("*~[CH2]~[#8]", 0), 110: ("[#7]~[#6]~[#8]", 0), 111: ("[#7]~*~[CH2]~*", 0),
    112: ("*~*(~*)(~*)~*", 0), 113: ("[#8]!:*:*", 0), 114: ("[CH3]~[CH2]~*", 0), 115: ("[CH3]~*~[CH2]~*", 0),
    117: ("[#7]~*~[#8]", 0), 119: ("[#7]=*", 0), 120: ("[!#6;R]", 1), 121: ("[#7;R]", 0),
    122: ("*~[#7](~*)~*", 0), 123: ("[#8]~[#6]~[#8]", 0), 124: (_Q + "~" + _Q, 0), 126: ("*!@[#8]!@*", 0),
    127: ("*@*!@[#8]", 1), 130: (_Q + "~" + _Q, 1), 131: (_QH, 1),
    132: ("[#8]~*~[CH2]~*", 0), 133: ("*@*!@[#7]", 0), 134: (_X, 0), 135: ("[#7]!:*:*", 0),
    136: ("[#8]=*", 1), 137: ("[!C;!c;R]", 0), 138: (_Q + "~[CH2]~*", 1), 139: ("[O;!H0]", 0),
    140: ("[#8]", 3), 141: ("[CH3]", 2), 142: ("[#7]", 1), 143: ("*@*!@[#8]", 0),
    144: ("*!:*:*!:*", 0), 145: ("*1~*~*~*~*~*~1", 1), 146: ("[#8]", 2), 148: ("*~" + _Q + "(~*)~*", 0),
    149: ("[C;H3,H4]", 1), 150: ("*!@*@*!@*", 0), 151: ("[#7;!H0]", 0), 152: ("[#8]~[#6](~[#6])~[#6]", 0),
    153: (_Q + "~[CH2]~*", 0), 154: ("[#6]=[#8]", 0), 155: ("*!@[CH2]!@*", 0), 156: ("[#7]~*(~*)~*", 0),
    157: ("[#6]-[#8]", 0), 158: ("[#6]-[#7]", 0), 159: ("[#8]", 1), 160: ("[C;H3,H4]", 0),
    161: ("[#7]", 0), 162: ("a", 0), 163: ("*1~*~*~*~*~*~1", 0), 164: ("[#8]", 0), 165: ("[R]", 0),
}

# keys that RDKit writes as one recursive atom: the matches are the anchor atoms of the alternatives
_ANCHORED = {
    90: ([_QH + "~*~*~[CH2]~*", "[!#6;!#1;!H0;R]1@[R]@[R]@[CH2;R]1", _QH + "~[R]1@[R]@[CH2;R]1"], 0),
    91: ([_QH + "~*~*~*~[CH2]~*", "[!#6;!#1;!H0;R]1@[R]@[R]@[R]@[CH2;R]1", _QH + "~[R]1@[R]@[R]@[CH2;R]1", _QH + "~*~[R]1@[R]@[CH2;R]1"], 0),
    101: ([_cycle(size) for size in range(8, 15)], 0),
    116: (["[CH3]~*~*~[CH2]~*", "[CH3]~*1~*~[CH2]1"], 0),
    118: (["*~[CH2]~[CH2]~*", "*1~[CH2]~[CH2]1"], 1),
    128: (["*~[CH2]~*~*~*~[CH2]~*", "[R]1@[CH2;R]@[R]@[R]@[R]@[CH2;R]1", "*~[CH2]~[R]1@[R]@[R]@[CH2;R]1", "*~[CH2]~*~[R]1@[R]@[CH2;R]1"], 0),
    129: (["*~[CH2]~*~*~[CH2]~*", "[R]1@[CH2]@[R]@[R]@[CH2;R]1", "*~[CH2]~[R]1@[R]@[CH2;R]1"], 0),
    147: (["*~[CH2]~[CH2]~*", "[R]1@[CH2;R]@[CH2;R]1"], 0),
}


def _entry(key):
    if key in _SINGLE:
        text, threshold = _SINGLE[key]
        return (f"maccs {key}: {text}", [text], threshold)
    if key in _ANCHORED:
        texts, threshold = _ANCHORED[key]
        return (f"maccs {key}: atoms of {len(texts)} alternatives", list(texts), threshold)
    if key in SPECIAL:
        return (f"maccs {key}: {SPECIAL[key]}", None, 1)
    return (f"maccs {key}: constant 0", None, 0)


MACCS_KEYS = tuple(_entry(key) for key in range(1, NUM_KEYS + 1))
assert set(_SINGLE) | set(_ANCHORED) | set(SPECIAL) | CONSTANT_ZERO == set(range(1, NUM_KEYS + 1))
assert len(_SINGLE) + len(_ANCHORED) + len(SPECIAL) + len(CONSTANT_ZERO) == NUM_KEYS


def pattern_table():
    """The flat list of pattern texts behind the keys and how each key reads it: ``(texts, single [(key, column, threshold)], anchored
    [(key, [columns], threshold)])``.  A text that several keys share has one column."""
    texts, column = [], {}

    def col(text):
        if text not in column:
            column[text] = len(texts)
            texts.append(text)
        return column[text]
    single = [(key, col(text), threshold) for key, (text, threshold) in sorted(_SINGLE.items())]
    anchored = [(key, [col(t) for t in alternatives], threshold) for key, (alternatives, threshold) in sorted(_ANCHORED.items())]
    return texts, single, anchored
