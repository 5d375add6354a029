"""A confidence threshold taken from the restatement's own scores.

The calibrated synthetic weights of scales m and l put the best class logit of a frame near -3.6 (score 0.03): at the suite's usual conf = 0.1
nothing is detected and the selection path would only ever be tested on NaN rows.  The end-to-end tests of those scales therefore place the
threshold between the frames' best scores, so that both outcomes occur in one batch."""
import numpy as np


def oracle_conf(cls_o, logit_margin: float):
    """cls_o: the restatement's class logits [B, A, nc] (tensor or array).  -> (conf, detects): conf is the score midway between the two middle
    values of the frames' best scores, detects[b] whether frame b's best score lies above it.  Asserts what makes the threshold a fair one: at
    least one frame detects, at least one gives the NaN row, and no frame's best logit lies within logit_margin of the threshold's logit (a GPU
    result inside its own tolerance cannot land on the other side)."""
    cls = np.asarray(cls_o, dtype=np.float64)
    best = cls.reshape(cls.shape[0], -1).max(axis=1)
    score = 1.0 / (1.0 + np.exp(-best))
    s = np.sort(score)
    lo, hi = s[(len(s) - 1) // 2], s[(len(s) - 1) // 2 + 1]
    conf = float(0.5 * (lo + hi))
    thr = float(np.log(conf / (1.0 - conf)))
    detects = score > conf
    assert detects.any() and not detects.all(), (score, conf)
    assert np.abs(best - thr).min() > logit_margin, (best, thr, logit_margin)
    return conf, detects
