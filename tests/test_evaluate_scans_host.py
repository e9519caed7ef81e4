"""evaluate.evaluate_scans, the loop of the reference's test driver (test.py:192-262), with the device work stubbed: the file names
(with the appended '.png'), test_accuracy.json against mean_average_precision of the pooled lists, one timing per scan around the
predict call only, pooling across scans.  No device needed."""
import copy
import json
import os

from faster_rcnn import evaluate, utils_io


def box(cls, x1, y1, x2, y2, prob=None):
    out = {'class': cls, 'x1': x1, 'y1': y1, 'x2': x2, 'y2': y2}
    if prob is not None:
        out['prob'] = prob
    return out


# three scans: a directory-like path (the reference's records), a name that already ends in .png, one in capitals
RECORDS = [{'filepath': 'scans/site_a/panel_1', 'bboxes': [box('boat', 0, 0, 10, 10), box('human', 20, 20, 30, 30)]},
           {'filepath': 'scans/site_b/panel_2.png', 'bboxes': [box('boat', 50, 50, 60, 60)]},
           {'filepath': 'panel_3.PNG', 'bboxes': []}]
DETECTIONS = {'scans/site_a/panel_1': [box('boat', 0, 0, 10, 10, 0.9), box('human', 100, 100, 110, 110, 0.8)],
              'scans/site_b/panel_2.png': [box('boat', 0, 0, 10, 9, 0.95), box('boat', 50, 50, 60, 61, 0.6), box('animal', 1, 1, 5, 5, 0.7)],
              'panel_3.PNG': [box('human', 20, 20, 30, 31, 0.5)]}


class _Net:
    def __init__(self, log):
        self.log = log

    def predict_from_path(self, path):
        self.log.append(("predict", path))
        return copy.deepcopy(DETECTIONS[path])

    def draw_detections(self, img, dets, **kw):
        self.log.append(("draw", img, [d['class'] for d in dets], kw))
        return ("drawn", img)


def run(tmp_path, monkeypatch, **kw):
    log = []
    monkeypatch.setattr(utils_io, "get_image", lambda path, types, random_type=False, to_host=True: log.append(("image", path, list(types), random_type, to_host))
                        or ("map", path))
    monkeypatch.setattr(utils_io, "imwrite", lambda path, img, **k: log.append(("write", path, img)) or True)
    clock = iter(range(0, 1000, 5))
    monkeypatch.setattr("time.time", lambda: log.append(("clock",)) or next(clock))
    records = copy.deepcopy(RECORDS)
    return evaluate.evaluate_scans(_Net(log), records, str(tmp_path), **kw), log, records


def test_evaluate_scans_writes_one_map_per_scan_and_the_pooled_accuracy(tmp_path, monkeypatch):
    (accuracy, elapsed, paths), log, records = run(tmp_path, monkeypatch)
    names = ["panel_1.png", "panel_2.png", "panel_3.PNG"]
    assert paths == [os.path.join(str(tmp_path), "test", n) for n in names]
    assert os.path.isdir(tmp_path / "test")
    writes = [e for e in log if e[0] == "write"]
    assert [(e[1], e[2]) for e in writes] == [(p, ("drawn", ("map", r['filepath']))) for p, r in zip(paths, RECORDS)]
    assert [e[1:] for e in log if e[0] == "image"] == [(r['filepath'], ['blended_grey'], False, False) for r in RECORDS]
    draws = [e for e in log if e[0] == "draw"]
    assert [(e[1], e[2]) for e in draws] == [(("map", r['filepath']), [d['class'] for d in DETECTIONS[r['filepath']]]) for r in RECORDS]
    assert all(e[3] == dict(color=(255, 255, 255), thickness=8, labels=True, label_scale=3, inplace=True) for e in draws)

    # pooled over the scans: the reference's lists, in scan order
    all_dets = [d for r in RECORDS for d in copy.deepcopy(DETECTIONS[r['filepath']])]
    all_gt = [g for r in copy.deepcopy(RECORDS) for g in r['bboxes']]
    want = {k: float(v) for k, v in evaluate.mean_average_precision(all_dets, all_gt).items()}
    assert accuracy == want and all(type(v) is float for v in accuracy.values())
    assert (tmp_path / "test_accuracy.json").read_text() == json.dumps(want, indent=4)
    assert list(accuracy) == ["animal", "boat", "human", "mAP"]
    # pooling runs ACROSS scans: scan 2's first boat matches scan 1's ground-truth boat (the pooled lists carry no image identity), so
    # both boat boxes are matched; per scan the second one's IoU partner would be another
    assert [g['bbox_matched'] for r in records for g in r['bboxes']] == [True, True, True]
    per_scan = [evaluate.mean_average_precision(copy.deepcopy(DETECTIONS[r['filepath']]), copy.deepcopy(r['bboxes'])) for r in RECORDS]
    assert all(p != want for p in per_scan)


def test_one_timing_per_scan_around_the_predict_call_only(tmp_path, monkeypatch):
    (accuracy, elapsed, paths), log, _ = run(tmp_path, monkeypatch)
    assert elapsed == [5, 5, 5] and len([e for e in log if e[0] == "clock"]) == 6
    kinds = [e[0] for e in log]
    for k, kind in enumerate(kinds):
        if kind == "predict":
            assert kinds[k - 1] == "clock" and kinds[k + 1] == "clock"                        # nothing else between the two readings


def test_the_arguments_reach_the_calls(tmp_path, monkeypatch):
    (accuracy, elapsed, paths), log, _ = run(tmp_path, monkeypatch, viz_type='blended', treshold=0.99, labels=False, label_scale=2)
    assert [e[2] for e in log if e[0] == "image"] == [['blended']] * 3
    assert all(e[3]['labels'] is False and e[3]['label_scale'] == 2 for e in log if e[0] == "draw")
    all_dets = [d for r in RECORDS for d in copy.deepcopy(DETECTIONS[r['filepath']])]
    all_gt = [g for r in copy.deepcopy(RECORDS) for g in r['bboxes']]
    assert accuracy == {k: float(v) for k, v in evaluate.mean_average_precision(all_dets, all_gt, 0.99).items()}
    assert accuracy != {k: float(v) for k, v in evaluate.mean_average_precision(copy.deepcopy(all_dets), copy.deepcopy(all_gt), 0.5).items()}


def test_no_scans_at_all(tmp_path, monkeypatch):
    log = []
    monkeypatch.setattr(utils_io, "imwrite", lambda *a, **k: log.append(a))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                                         # the mean over no classes
        accuracy, elapsed, paths = evaluate.evaluate_scans(_Net(log), [], str(tmp_path))
    assert elapsed == [] and paths == [] and log == [] and list(accuracy) == ["mAP"]
    assert os.path.exists(tmp_path / "test_accuracy.json")
