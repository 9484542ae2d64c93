"""ClassificationTrainer with the reference's interface (model_trainers/ClassificationTrainer.py): a ModularTrainer
whose score is the accuracy of an utterance-level classifier.  `create_hparams` adds `class_pred_name`,
`class_true_name`, `num_classes` and `class_names`; `compute_score` returns

    W_acc        correct utterances / utterances (scikit-learn's accuracy_score)
    U_acc        mean over `num_classes` of the per-class recall: the diagonal of the row-normalised confusion matrix
    conf_matrix  [true class, predicted class] counts divided by the class's count, empty classes divided by 1

The reference's scikit-learn calls (confusion_matrix with labels = range(num_classes), accuracy_score) are restated
in numpy: a pair whose true or predicted class lies outside the labels is left out of the matrix, as there."""
import numpy as np

from idiaptts_amd.src.model_trainers.ModularTrainer import ModularTrainer


def confusion_counts(class_true, class_pred, num_classes):
    """[num_classes, num_classes] int64, entry [i, j] = samples of true class i predicted as j"""
    class_true = np.asarray(class_true).reshape(-1).astype(np.int64)
    class_pred = np.asarray(class_pred).reshape(-1).astype(np.int64)
    inside = (class_true >= 0) & (class_true < num_classes) & (class_pred >= 0) & (class_pred < num_classes)
    conf_matrix = np.zeros((num_classes, num_classes), dtype=np.int64)
    np.add.at(conf_matrix, (class_true[inside], class_pred[inside]), 1)
    return conf_matrix


class ClassificationTrainer(ModularTrainer):

    @staticmethod
    def create_hparams(hparams_string=None, verbose=False):
        hparams = ModularTrainer.create_hparams(hparams_string=hparams_string, verbose=verbose)
        hparams.add_hparams(
            class_pred_name="class_pred",
            class_true_name="class_true",
            num_classes=-1,
            class_names=None)
        return hparams

    def compute_score(self, data, output, hparams):
        """`output`: {id: {class_pred_name: logits of the utterance, class_true_name: its class index}} (:34-59)"""
        n_cls = hparams.num_classes
        pred = np.array([np.asarray(o[hparams.class_pred_name]).argmax() for o in output.values()], dtype=np.int64)
        true = np.array([int(np.asarray(o[hparams.class_true_name]).squeeze()) for o in output.values()],
                        dtype=np.int64)
        counts = confusion_counts(true, pred, n_cls)
        conf_matrix = counts / np.maximum(counts.sum(axis=1, keepdims=True), 1)      # empty classes: divided by 1
        scores = {"W_acc": float(np.mean(true == pred)),
                  "U_acc": float(np.trace(conf_matrix) / n_cls),
                  "conf_matrix": conf_matrix}
        self.logger.info("Weighted accuracy {}".format(scores["W_acc"]))
        self.logger.info("Unweighted accuracy {}".format(scores["U_acc"]))
        self.logger.info("Confusion matrix\n{}\n{}".format(
            hparams.class_names if hparams.class_names is not None else "", conf_matrix))
        return scores
