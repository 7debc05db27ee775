# Same command line as the reference's segmentation baseline run (main_ori.py on VOC 2012, DeepLabv3+ ResNet-50, batch 4): the mIoU the
# A-FAN runs of run_seg.sh are compared against.  Run from cv_a-fan_amd/ like the reference runs from Segmentation/.
# Without the data: add --synthetic 64 (random images; a second synthetic split is validated on).
GPU=0
EXP=baseline_voc2012_resnet50_bs4_seed66

python -u main_ori.py --year 2012 --crop_val --batch_size 4 \
--model deeplabv3plus_resnet50 \
--gpu_id ${GPU} \
--random_seed 66 \
${EXP}

# Cityscapes (19 classes, 768 x 768 crops with colour jitter, lr 0.1), the settings of the reference's Cityscapes runs:
# python -u main_ori.py --model deeplabv3plus_resnet50 --data_root ./datasets/data/cityscapes --dataset cityscapes \
# --lr 0.1 --crop_size 768 --batch_size 4 --gpu_id ${GPU} baseline_city_resnet50_bs4
