"""PairsDataLoader's host logic restated in plain Python from its definition (test infrastructure only):
reading and splitting a pairs file, and the word pairs of one epoch as a function of Python's `random` state."""
import random


def read_pairs(pairs_path, id_to_file=None):
    names = {}
    if id_to_file is not None:
        for line in open(id_to_file):
            fid, name = line.split()
            names[int(fid)] = name
    pairs = []
    for line in open(pairs_path):
        f = line.split(' ')
        assert len(f) == 7
        f1, f2 = int(f[0]), int(f[1])
        pairs.append([names.get(f1, f1), int(f[2]), int(f[3]), names.get(f2, f2), int(f[4]), int(f[5])])
    return pairs


def split_each_file(pairs, ratio):
    longest = {}
    for f1, _, e1, f2, _, e2 in pairs:
        longest[f1] = max(longest.get(f1, 0), e1)
        longest[f2] = max(longest.get(f2, 0), e2)
    train, test = [], []
    for p in pairs:
        c1, c2 = longest[p[0]] * ratio, longest[p[3]] * ratio
        if p[1] > c1 and p[4] > c2:
            test.append(p)
        elif p[1] < c1 and p[4] <= c2:
            train.append(p)
    return train, test


def split_files(pairs, ratio):
    """Draws from `random`: the test files are a sample of the sorted file list."""
    files = sorted({p[0] for p in pairs} | {p[3] for p in pairs})
    test_files = set(random.sample(files, int(len(files) * (1 - ratio))))
    train = [p for p in pairs if p[0] not in test_files and p[3] not in test_files]
    test = [p for p in pairs if p[0] in test_files and p[3] in test_files]
    return train, test


def tokens_of(pairs):
    """In the iteration order of a set filled in the pairs' order (what random.choices later indexes)."""
    seen = set()
    for p in pairs:
        seen.add((p[0], p[1], p[2]))
        seen.add((p[3], p[4], p[5]))
    return list(seen)


def epoch_pairs(positives, tokens, iterations, batch_size, proportion_positive):
    total = iterations * batch_size
    n_pos = min(int(total * proportion_positive), len(positives))
    n_neg = total - n_pos
    pos = [list(p) + ['same'] for p in random.sample(positives, n_pos)]
    drawn = random.choices(tokens, k=2 * n_neg)
    neg = [list(drawn[2 * i]) + list(drawn[2 * i + 1]) + ['diff'] for i in range(n_neg)]
    pairs = pos + neg
    random.shuffle(pairs)
    return pairs


def batches(pairs, iterations, batch_size):
    out = []
    for i in range(iterations):
        b = pairs[i * batch_size:(i + 1) * batch_size]
        if not b:
            break
        out.append(b)
    return out
