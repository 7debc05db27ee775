# Segmentation PGD training (the reference's main_advtrain.py) on VOC 2012, DeepLabv3+ ResNet-50, batch 4 (the only batch size the
# reference's loop accepts): image-space sign-PGD on every batch with the model in training mode, one SGD step on the adversarial
# images; checkpoints under adv_training/${EXP}/.  eps / gamma are in /255 pixel units.  Run from cv_a-fan_amd/ like the reference runs
# from Segmentation/.  Without the data: add --synthetic 64 (random images; a second synthetic split is validated on).
# --noise host draws --randinit_pgd's start on the CPU generator, as the reference does (eager); the default draws it on the device.
GPU=0
EXP=advtrain_voc2012_resnet50_bs4_seed66

python -u main_advtrain.py --year 2012 --crop_val --batch_size 4 \
--model deeplabv3plus_resnet50 \
--gpu_id ${GPU} \
--random_seed 66 \
--steps_pgd 1 --eps_pgd 2 --gamma_pgd 0.5 --randinit_pgd --clip_pgd \
${EXP}

# Clean and robust scores of the checkpoint it wrote (the same evaluations as cmd/run_seg_val.sh and cmd/run_seg_rob.sh):
# CKPT=adv_training/${EXP}/best_deeplabv3plus_resnet50_voc_os16.pth
# python -u main_advtrain.py --year 2012 --crop_val --gpu_id ${GPU} --test_only ${CKPT} ${EXP}
# python -u main_advtrain.py --year 2012 --crop_val --gpu_id ${GPU} --steps_pgd 3 --eps_pgd 8 --gamma_pgd 2 --clip_pgd --eval_pgd ${CKPT} ${EXP}
