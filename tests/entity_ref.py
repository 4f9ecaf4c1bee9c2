"""The obvious sequential BIO decoder and entity matcher that the entity tests compare against: one loop per row,
entities into a Python set, common = |set_a & set_b|.  Written from the rule alone and importing nothing of the
package, so that it shares no code with polus_amd/ner/bio.py or the kernels.

scheme[tag] = -1 for an outside tag, else 2 * type + (1 for I-).  Masked-out tokens (mask == 0) are skipped as if they
were not there.  A kept id outside [0, C) is outside and counted as rejected."""


def decode_row(tags, scheme, mask=None):
    """([(start, end_exclusive, type), ...] in order of start,
        {"tags", "rejected", "inside_tag_after_other_tag", "inside_tag_with_different_entity_type"}) of one row."""
    C = len(scheme)
    stats = {"tags": 0, "rejected": 0, "inside_tag_after_other_tag": 0, "inside_tag_with_different_entity_type": 0}
    entities = []
    open_start = open_end = open_type = None       # the entity being built
    for col, tag in enumerate(tags):
        if mask is not None and not mask[col]:
            continue
        stats["tags"] += 1
        tag = int(tag)
        if 0 <= tag < C:
            code = int(scheme[tag])
        else:
            code = -1
            stats["rejected"] += 1
        if code < 0:                               # O
            if open_type is not None:
                entities.append((open_start, open_end, open_type))
            open_type = None
            continue
        typ, inside_tag = code // 2, code % 2 == 1
        if inside_tag and open_type == typ:        # I- that goes on
            open_end = col + 1
            continue
        if inside_tag:                             # I- that has to start an entity: lenient decoding
            if open_type is None:
                stats["inside_tag_after_other_tag"] += 1
            else:
                stats["inside_tag_with_different_entity_type"] += 1
        if open_type is not None:
            entities.append((open_start, open_end, open_type))
        open_start, open_end, open_type = col, col + 1, typ
    if open_type is not None:
        entities.append((open_start, open_end, open_type))
    return entities, stats


def decode(tags, scheme, mask=None):
    """Per row the entity list, and the statistics summed over rows."""
    rows, total = [], None
    for r in range(len(tags)):
        ents, st = decode_row(tags[r], scheme, None if mask is None else mask[r])
        rows.append(ents)
        total = st if total is None else {k: total[k] + st[k] for k in st}
    if total is None:
        total = {"tags": 0, "rejected": 0, "inside_tag_after_other_tag": 0, "inside_tag_with_different_entity_type": 0}
    return rows, total


def counts_from_decoded(rows_a, st_a, rows_b, st_b, num_types):
    """(counts, stats) of entity_counts from what decode() returned for the two sides."""
    counts = [[0, 0, 0] for _ in range(num_types)]
    for r, (ea, eb) in enumerate(zip(rows_a, rows_b)):
        sa, sb = {(r,) + e for e in ea}, {(r,) + e for e in eb}
        assert len(sa) == len(ea) and len(sb) == len(eb)
        for e in sa & sb:
            counts[e[3]][0] += 1
        for e in sa:
            counts[e[3]][1] += 1
        for e in sb:
            counts[e[3]][2] += 1
    stats = [st_a["tags"], st_a["rejected"] + st_b["rejected"],
             st_a["inside_tag_after_other_tag"], st_a["inside_tag_with_different_entity_type"],
             st_b["inside_tag_after_other_tag"], st_b["inside_tag_with_different_entity_type"]]
    return counts, stats


def entity_counts(tags_a, tags_b, scheme, num_types, mask=None):
    """(counts [T][3] = per type (common, n_a, n_b), stats [6] = kept tokens, rejected of both, the two decode
    statistics of a, then of b) as lists of Python ints."""
    rows_a, st_a = decode(tags_a, scheme, mask)
    rows_b, st_b = decode(tags_b, scheme, mask)
    return counts_from_decoded(rows_a, st_a, rows_b, st_b, num_types)


def micro_f1(counts):
    tp = sum(c[0] for c in counts)
    fn = sum(c[1] for c in counts) - tp
    fp = sum(c[2] for c in counts) - tp
    den = tp + 0.5 * (fp + fn)
    return tp / den if den else 0.0
