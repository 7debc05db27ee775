# Evaluate a trained ResNet-56s checkpoint on the CIFAR-10 test split (run from this directory).
# --pretrained: a checkpoint.pt / best_model.pt written by main_perturb.py, or one in the reference's layout.
python -u main_inference.py --pretrained res56s_adv_aug/best_model.pt --data ../data --batch_size 128 --print_freq 50
