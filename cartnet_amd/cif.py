"""A small CIF reader: what the symmetry expansion (cartnet_amd/symmetry.py) needs of a crystallographic file.

The reference builds its dataset through the CSD Python API (dataset/extract_csd_data.py:44-143), which needs a licence.
A CIF stores the same information: an asymmetric unit, the symmetry operators, the cell and the ``U_ij``.  ``read_cif``
returns one ``CifCrystal`` per data block; ``CifCrystal.reject_reason`` applies the reference's filters (:49-56, :95-97).
There is no space-group table: the operators must be in the file (or the block must declare P1).  Pure Python, no
third-party parser.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Dict, List, Optional, Tuple

import numpy as np

from .predict import SYMBOLS

_Z = {s.upper(): z for z, s in enumerate(SYMBOLS) if z > 0}
_Z["D"] = 1                                                    # deuterium
_NUMBER = re.compile(r"^([+-]?(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?)(?:\(\d+\))?$")
_OP_TAGS = ("_space_group_symop_operation_xyz", "_symmetry_equiv_pos_as_xyz")
_ANISO = tuple("_atom_site_aniso_u_" + k for k in ("11", "22", "33", "23", "13", "12"))


class CifError(ValueError):
    pass


def _tokens(text: str) -> List[Tuple[str, str]]:
    """(kind, value) with kind 'w' (a bare word: tag, keyword or value) or 's' (quoted string / text field)."""
    out: List[Tuple[str, str]] = []
    lines = text.replace("\r\n", "\n").replace("\r", "\n").split("\n")
    k = 0
    while k < len(lines):
        line = lines[k]
        if line.startswith(";"):                                # a semicolon text field runs to the next line starting with ;
            body = [line[1:]]
            k += 1
            while k < len(lines) and not lines[k].startswith(";"):
                body.append(lines[k])
                k += 1
            if k == len(lines):
                raise CifError("unterminated semicolon text field")
            out.append(("s", "\n".join(body).strip()))
            line = lines[k][1:]
        i, n = 0, len(line)
        while i < n:
            c = line[i]
            if c in " \t":
                i += 1
            elif c == "#":
                break
            elif c in "'\"":                                    # closes at the same quote followed by whitespace or the end
                j = i + 1
                while j < n and not (line[j] == c and (j + 1 == n or line[j + 1] in " \t")):
                    j += 1
                if j >= n:
                    raise CifError(f"unterminated quoted string: {line.strip()}")
                out.append(("s", line[i + 1:j]))
                i = j + 1
            else:
                j = i
                while j < n and line[j] not in " \t":
                    j += 1
                out.append(("w", line[i:j]))
                i = j
        k += 1
    return out


def _blocks(text: str) -> List[Tuple[str, Dict[str, str], List[Tuple[List[str], List[List[str]]]]]]:
    """[(block name, {tag: value}, [(loop tags, rows)])]; tags in lower case."""
    toks = _tokens(text)
    blocks = []
    pairs: Optional[Dict[str, str]] = None
    loops: List = []
    i = 0

    def is_tag(t):
        return t[0] == "w" and t[1].startswith("_")

    def is_value(t):
        return t[0] == "s" or not (t[1].startswith("_") or t[1].lower().startswith(("data_", "save_", "global_"))
                                   or t[1].lower() in ("loop_", "stop_"))
    while i < len(toks):
        kind, val = toks[i]
        low = val.lower()
        if kind == "w" and low.startswith("data_"):
            pairs, loops = {}, []
            blocks.append((val[5:], pairs, loops))
            i += 1
        elif kind == "w" and low.startswith("save_"):
            i += 1
        elif pairs is None:
            raise CifError(f"'{val}' before the first data_ block")
        elif kind == "w" and low == "loop_":
            i += 1
            tags = []
            while i < len(toks) and is_tag(toks[i]):
                tags.append(toks[i][1].lower())
                i += 1
            vals = []
            while i < len(toks) and is_value(toks[i]):
                vals.append(toks[i][1])
                i += 1
            if not tags or len(vals) % len(tags):
                raise CifError(f"loop of {tags[:1]}...: {len(vals)} values for {len(tags)} tags")
            loops.append((tags, [vals[r:r + len(tags)] for r in range(0, len(vals), len(tags))]))
        elif is_tag(toks[i]):
            if i + 1 >= len(toks) or not is_value(toks[i + 1]):
                raise CifError(f"tag {val} without a value")
            pairs[low] = toks[i + 1][1]
            i += 2
        else:
            raise CifError(f"value '{val}' without a tag")
    return blocks


def number(s: Optional[str]) -> Optional[float]:
    """A CIF number, its esd dropped (``0.1234(5)`` -> 0.1234); None for ``?``, ``.`` and None."""
    if s is None or s in ("?", "."):
        return None
    m = _NUMBER.match(s.strip())
    if not m:
        raise CifError(f"not a number: '{s}'")
    return float(m.group(1))


def parse_symop(text: str) -> Tuple[np.ndarray, np.ndarray]:
    """``"-x+1/2, y+1/2, -z"`` -> (W int64 [3,3] with entries in {-1, 0, 1} and |det W| = 1, w float64 [3]); the
    translations are exact fractions (``1/3`` is the fp64 nearest to one third)."""
    parts = text.strip().lower().replace(" ", "").split(",")
    if len(parts) != 3:
        raise CifError(f"symmetry operator '{text}': expected three components")
    W = np.zeros((3, 3), dtype=np.int64)
    w = [Fraction(0)] * 3
    for r, comp in enumerate(parts):
        terms = re.findall(r"[+-]?[^+-]+", comp)
        if not terms or "".join(terms) != comp:
            raise CifError(f"symmetry operator '{text}': cannot read '{comp}'")
        for t in terms:
            sign = -1 if t[0] == "-" else 1
            body = t.lstrip("+-")
            if body in ("x", "y", "z"):
                W[r, "xyz".index(body)] += sign
            elif re.fullmatch(r"\d+(/\d+)?|\d*\.\d+", body):
                w[r] += sign * Fraction(body)
            else:
                raise CifError(f"symmetry operator '{text}': cannot read the term '{t}'")
    if np.abs(W).max() > 1:
        raise CifError(f"symmetry operator '{text}': a rotation entry outside -1, 0, 1")
    if abs(int(round(np.linalg.det(W)))) != 1:
        raise CifError(f"symmetry operator '{text}': the rotation part is singular")
    return W, np.array([float(t) for t in w], dtype=np.float64)


def format_symop(W, w) -> str:
    """The inverse of ``parse_symop`` for translations that are multiples of 1/24 (others are printed as decimals)."""
    out = []
    for r in range(3):
        s = ""
        for c in range(3):
            v = int(W[r][c])
            if v:
                s += ("-" if v < 0 else "+" if s else "") + "xyz"[c]
        t = Fraction(float(w[r])).limit_denominator(48)
        if abs(float(t) - float(w[r])) > 1e-12:
            s += f"{float(w[r]):+.10f}"
        elif t:
            s += ("+" if t > 0 else "-") + (f"{abs(t.numerator)}/{t.denominator}" if t.denominator != 1 else f"{abs(t.numerator)}")
        out.append(s or "0")
    return ",".join(out)


def cell_matrix(a: float, b: float, c: float, alpha: float, beta: float, gamma: float) -> np.ndarray:
    """The cell in fp64, rows = the lattice vectors, in the convention of the reference's ``frac_to_cart_matrix``
    (dataset/extract_csd_data.py:15-25): a along x, b in the xy plane; angles in degrees."""
    with np.errstate(all="ignore"):                              # a degenerate cell comes out singular or not finite
        a, b, c = (np.float64(v) for v in (a, b, c))
        al, be, ga = (np.radians(np.float64(v)) for v in (alpha, beta, gamma))
        ca, cb, cg, sg = np.cos(al), np.cos(be), np.cos(ga), np.sin(ga)
        vol = c * np.sqrt(1.0 - ca * ca - cb * cb - cg * cg + 2.0 * ca * cb * cg) * b * a
        return np.array([[a, 0.0, 0.0],
                         [b * cg, b * sg, 0.0],
                         [c * cb, c * (ca - cb * cg) / sg, vol / (a * b * sg)]], dtype=np.float64)


@dataclass
class CifCrystal:
    name: str
    cell_parameters: Optional[Tuple[float, ...]] = None          # a, b, c, alpha, beta, gamma
    temperature: Optional[float] = None                           # Kelvin
    pressure: Optional[float] = None
    symops: List[Tuple[np.ndarray, np.ndarray]] = field(default_factory=list)   # identity first
    symop_strings: List[str] = field(default_factory=list)
    labels: List[str] = field(default_factory=list)
    symbols: List[str] = field(default_factory=list)
    z: List[int] = field(default_factory=list)
    frac: List[Tuple[float, float, float]] = field(default_factory=list)
    occupancy: List[Optional[float]] = field(default_factory=list)
    disorder_group: List[str] = field(default_factory=list)
    u_iso: List[Optional[float]] = field(default_factory=list)
    adp_type: List[Optional[str]] = field(default_factory=list)
    u_aniso: Dict[str, Tuple[float, ...]] = field(default_factory=dict)          # label -> U11 U22 U33 U23 U13 U12
    aniso_in_b: bool = False
    problem: Optional[str] = None                                 # a defect of the block found while reading it

    def cell(self) -> np.ndarray:
        return cell_matrix(*self.cell_parameters)

    def u_cif(self) -> np.ndarray:
        """[n,6] fp64, NaN where the atom has no aniso row."""
        nan = (float("nan"),) * 6
        return np.array([self.u_aniso.get(lab, nan) for lab in self.labels], dtype=np.float64).reshape(-1, 6)

    def reject_reason(self, labeled: bool, temperature: Optional[float] = None) -> Optional[str]:
        """Why this crystal cannot be used, or None: the reference's filters (dataset/extract_csd_data.py:49-56, :95-97) and
        what the expansion needs.  ``temperature``: a default for blocks that give none.  Hydrogens never need ADPs."""
        if self.problem:
            return self.problem
        if self.cell_parameters is None:
            return "no cell"
        if not self.labels:
            return "no atoms"
        if self.pressure is not None:
            return "pressure given"
        if any(g not in (".", "?") for g in self.disorder_group) or any(o is not None and o < 1.0 for o in self.occupancy):
            return "disorder"
        if self.temperature is None and temperature is None:
            return "no temperature"
        if not self.symops:
            return "no operators"
        if any(v <= 0 for v in self.z):
            return "unknown element"
        if labeled:
            if self.aniso_in_b:
                return "aniso loop in B"
            for lab, v in zip(self.labels, self.z):
                if v != 1 and lab not in self.u_aniso:
                    return f"non-hydrogen atom {lab} without anisotropic ADPs"
        return None


def _element(symbol: Optional[str], label: str) -> Tuple[str, int]:
    """(symbol, Z) from the type symbol (a charge is ignored), else from the alphabetic prefix of the label: the whole
    prefix if it is an element, else its first two letters, else its first; ("X", 0) if nothing fits."""
    for cand in (symbol, label):
        m = re.match(r"[A-Za-z]+", cand) if cand and cand not in ("?", ".") else None
        if m:
            s = m.group(0).upper()
            for t in (s, s[:2], s[:1]):
                if t in _Z:
                    return ("D" if t == "D" else t.capitalize()), _Z[t]
    return "X", 0


def _crystal(name: str, pairs: Dict[str, str], loops) -> CifCrystal:
    c = CifCrystal(name=name)
    try:
        cp = [number(pairs.get(t)) for t in ("_cell_length_a", "_cell_length_b", "_cell_length_c", "_cell_angle_alpha",
                                             "_cell_angle_beta", "_cell_angle_gamma")]
        if all(v is not None for v in cp):
            c.cell_parameters = tuple(cp)
        t = pairs.get("_diffrn_ambient_temperature")
        if t is not None:                                         # the first number in the field (extract_csd_data.py:64-68)
            m = re.findall(r"\d+\.?\d*", t)
            c.temperature = float(m[0]) if m else None
        p = pairs.get("_diffrn_ambient_pressure")
        if p not in (None, "?", "."):                             # given, whatever it says
            c.pressure = number(p) if _is_number(p) else float("nan")

        def column(tags, row, tag):
            return row[tags.index(tag)] if tag in tags else None
        ops: List[str] = []
        for tags, rows in loops:
            for tag in _OP_TAGS:
                if tag in tags:
                    ops = [column(tags, r, tag) for r in rows]
            if "_atom_site_label" in tags and "_atom_site_fract_x" in tags:
                for r in rows:
                    lab = column(tags, r, "_atom_site_label")
                    sym, z = _element(column(tags, r, "_atom_site_type_symbol"), lab)
                    xyz = tuple(number(column(tags, r, "_atom_site_fract_" + k)) for k in "xyz")
                    if any(v is None for v in xyz):
                        c.problem = f"atom {lab} without coordinates"
                        xyz = (float("nan"),) * 3
                    c.labels.append(lab)
                    c.symbols.append(sym)
                    c.z.append(z)
                    c.frac.append(xyz)
                    c.occupancy.append(number(column(tags, r, "_atom_site_occupancy")))
                    c.disorder_group.append(column(tags, r, "_atom_site_disorder_group") or ".")
                    c.u_iso.append(number(column(tags, r, "_atom_site_u_iso_or_equiv")))
                    c.adp_type.append(column(tags, r, "_atom_site_adp_type"))
            if "_atom_site_aniso_label" in tags:
                if any(t.startswith("_atom_site_aniso_b_") for t in tags):
                    c.aniso_in_b = True
                if all(t in tags for t in _ANISO):
                    for r in rows:
                        u = tuple(number(column(tags, r, t)) for t in _ANISO)
                        if all(v is not None for v in u):
                            c.u_aniso[column(tags, r, "_atom_site_aniso_label")] = u
        for tag in _OP_TAGS:                                      # a single operator may be given outside a loop
            if not ops and tag in pairs:
                ops = [pairs[tag]]
        if not ops and _declares_p1(pairs):
            ops = ["x,y,z"]
        parsed = [(s,) + parse_symop(s) for s in ops]
        ident = [k for k, (_, W, w) in enumerate(parsed) if np.array_equal(W, np.eye(3, dtype=np.int64)) and not w.any()]
        if parsed and not ident:
            c.problem = "the identity is not among the operators"
        elif parsed:
            parsed.insert(0, parsed.pop(ident[0]))
            c.symop_strings = [p[0] for p in parsed]
            c.symops = [(p[1], p[2]) for p in parsed]
    except CifError as e:
        c.problem = str(e)
    return c


def _is_number(s: Optional[str]) -> bool:
    return s is not None and s not in ("?", ".") and _NUMBER.match(s.strip()) is not None


def _declares_p1(pairs: Dict[str, str]) -> bool:
    for tag in ("_symmetry_space_group_name_h-m", "_space_group_name_h-m_alt"):
        if pairs.get(tag, "").replace(" ", "").upper() == "P1":
            return True
    for tag in ("_symmetry_int_tables_number", "_space_group_it_number"):
        if _is_number(pairs.get(tag)) and number(pairs[tag]) == 1:
            return True
    return False


def read_cif(path_or_text: str) -> List[CifCrystal]:
    """One ``CifCrystal`` per data block of a file (or of the text itself, if it contains a line break).  A block that
    cannot be understood is returned with ``problem`` set, which ``reject_reason`` reports; broken syntax raises
    ``CifError``."""
    text = path_or_text
    if "\n" not in path_or_text:
        with open(path_or_text, "r", errors="replace") as f:
            text = f.read()
    return [_crystal(name, pairs, loops) for name, pairs, loops in _blocks(text)]


def find_cifs(paths) -> List[str]:
    """The ``.cif`` files named by ``paths``: files as given, directories listed (sorted, not recursive)."""
    out = []
    for p in ([paths] if isinstance(paths, str) else paths):
        if os.path.isdir(p):
            out += [os.path.join(p, f) for f in sorted(os.listdir(p)) if f.lower().endswith(".cif")]
        else:
            out.append(p)
    return out


def load_crystals(paths, labeled: bool, temperature: Optional[float] = None):
    """Every data block of the CIF files named by ``paths`` (``find_cifs``): ``(accepted, rejected)`` with ``accepted`` a
    list of ``CifCrystal`` whose names are unique (a block without a name takes the file's; a repeated name gets a
    running number) and ``rejected`` a list of ``(name, reason)``: ``reject_reason`` or what made the file unreadable."""
    accepted: List[CifCrystal] = []
    rejected: List[Tuple[str, str]] = []
    seen: Dict[str, int] = {}
    for path in find_cifs(paths):
        stem = os.path.splitext(os.path.basename(path))[0]
        try:
            blocks = read_cif(path)
        except (CifError, OSError) as e:
            rejected.append((stem, str(e)))
            continue
        for c in blocks:
            c.name = c.name or stem
            seen[c.name] = seen.get(c.name, 0) + 1
            if seen[c.name] > 1:
                c.name = f"{c.name}_{seen[c.name]}"
            why = c.reject_reason(labeled, temperature)
            if why is None:
                accepted.append(c)
            else:
                rejected.append((c.name, why))
    return accepted, rejected
