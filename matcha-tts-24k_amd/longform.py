"""Texts longer than one utterance, host side: a text cut into the segments that are spoken as rows of one ragged batch and joined on
the device (``FrameBudgetBatcher.submit_document``, ``inference.to_waveforms(documents=...)``).  Pure Python, no device.

The reference speaks one utterance per request and refuses a longer text (server.py:31,94-96), so there is nothing to take the
pauses or the limits from: they are parameters.  This is a splitter, not a text normaliser: the rows have no prosody across
sentences, no token-level marks are added, and the abbreviation sets are a handful of titles per language, not a dictionary.
"""
from __future__ import annotations

import re
from typing import Iterable, List, Optional, Tuple

TERMINATORS = ".!?…"                    # a run of these ends a sentence ...
CLOSERS = "\"'”’»)]}"         # ... with the quotes and brackets that close behind it
CLAUSE_MARKS = ",;:—"                   # where a sentence that is too long is cut first
OPENERS = "\"'“‘«([{"

#: tokens after which a single full stop does not end a sentence, by the first two letters of the voice's language
ABBREVIATIONS = {
    "en": ("Mr", "Mrs", "Ms", "Dr", "Prof", "Sr", "Jr", "St", "vs", "etc", "e.g", "i.e", "No", "Fig", "cf"),
    "de": ("Dr", "Prof", "Hr", "Fr", "Nr", "z.B", "d.h", "u.a", "bzw", "ca", "usw", "St"),
    "fr": ("M", "Mme", "Mlle", "Dr", "Pr", "St", "cf", "p.ex", "etc"),
    "es": ("Sr", "Sra", "Srta", "Dr", "Dra", "Ud", "Uds", "p.ej", "etc"),
}


def normalise_space(text: str) -> str:
    """Runs of whitespace as single spaces, none at the ends: what the segments of ``split_text``, joined by spaces, give back."""
    return " ".join(text.split())


def split_sentences(paragraph: str, abbreviations: Iterable[str] = ()) -> List[str]:
    """The sentences of one paragraph (whitespace normalised): a sentence ends after a run of ``. ! ? ...`` and the quotes or brackets
    closing behind it when a space follows -- unless the next character is a lowercase letter or a digit, or the run is a single
    full stop behind one of ``abbreviations``.  The terminator stays with its sentence."""
    s = normalise_space(paragraph)
    known = set(abbreviations)
    out, start, i, n = [], 0, 0, len(s)
    while i < n:
        if s[i] not in TERMINATORS:
            i += 1
            continue
        j = i
        while j < n and s[j] in TERMINATORS:
            j += 1
        k = j
        while k < n and s[k] in CLOSERS:
            k += 1
        if k < n and s[k] == " ":
            nxt = s[k + 1]                               # (normalised: a space is never the last character)
            token = s[s.rfind(" ", 0, i) + 1:i].lstrip(OPENERS)
            abbreviated = j == i + 1 and s[i] == "." and token in known
            if not (nxt.islower() or nxt.isdigit()) and not abbreviated:
                out.append(s[start:k])
                start = k + 1
        i = max(k, i + 1)
    if start < n:
        out.append(s[start:])
    return out


def split_long(sentence: str, max_chars: int, clause_ms: float) -> List[Tuple[str, Optional[float]]]:
    """A sentence of more than ``max_chars`` characters in pieces of at most that many: cut behind the last ``, ; : --`` (followed by
    a space) that leaves a piece within the limit, with the clause pause; failing that at the last space, with pause 0.  A word
    longer than the limit stays whole.  The last piece's pause is None: the caller's."""
    out, s = [], sentence
    while len(s) > max_chars:
        cut, pause = -1, 0.0
        for idx in range(min(max_chars, len(s) - 1) - 1, -1, -1):
            if s[idx] in CLAUSE_MARKS and s[idx + 1] == " ":
                cut, pause = idx + 1, float(clause_ms)
                break
        if cut < 0:
            cut = s.rfind(" ", 1, max_chars + 1)
        if cut < 0:
            cut = s.find(" ", max_chars)
        if cut < 0:
            break
        out.append((s[:cut], pause))
        s = s[cut + 1:]
    out.append((s, None))
    return out


def split_text(text: str, max_chars: int = 300, sentence_ms: float = 300.0, paragraph_ms: float = 600.0, clause_ms: float = 120.0,
               abbreviations: Optional[Iterable[str]] = None, language: str = "en") -> List[Tuple[str, float]]:
    """``text`` as ``[(segment, pause_ms)]`` in speaking order: paragraphs split at blank lines, sentences by ``split_sentences``,
    a sentence above ``max_chars`` by ``split_long``.  The pause is the silence after the segment: ``paragraph_ms`` behind the last
    sentence of a paragraph, ``sentence_ms`` behind any other sentence, ``clause_ms`` or 0 inside a sentence that was cut.
    ``abbreviations``: the tokens a full stop does not end a sentence after (default: ``ABBREVIATIONS`` of ``language``).
    The segments joined by single spaces are the whitespace-normalised text: no character is lost or invented."""
    if int(max_chars) < 1:
        raise ValueError("max_chars must be at least 1")
    if abbreviations is None:
        abbreviations = ABBREVIATIONS.get(str(language).lower()[:2], ())
    abbreviations = tuple(abbreviations)
    out: List[Tuple[str, float]] = []
    for paragraph in re.split(r"\n[^\S\n]*\n\s*", text):
        sentences = split_sentences(paragraph, abbreviations)
        for n, sentence in enumerate(sentences):
            after = float(paragraph_ms) if n == len(sentences) - 1 else float(sentence_ms)
            for piece, pause in split_long(sentence, int(max_chars), clause_ms):
                out.append((piece, after if pause is None else pause))
    return out
